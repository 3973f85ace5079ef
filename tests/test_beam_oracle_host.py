"""The fp64 beam search the GPU tests compare against (tests/beam_oracle.py) is itself pinned on the CPU:

* K = 1 is decoder_forward's greedy decode: the same tokens, and exactly its sum_t log token_probs;
* exhaustive: at T_dec = 6 the CLEVR automaton accepts 1152 complete layouts (counted below; 6 / 40 / 214 at
  T_dec = 3 / 4 / 5) and never more valid prefixes at an earlier step, so a beam of width 1152 keeps every
  prefix -- its best beam must be the arg-max over ALL layouts scored one by one with
  decoder_forward(forced_tokens=...), for every question, and its score the true maximum;
* every returned beam's score is reproduced to 1e-12 by decoder_forward(forced_tokens=beam);
* the <eos> latch (all-valid tables): every beam is <eos> behind its first <eos> and its score counts the steps
  in front of and including that <eos> only.
"""
import dataclasses

import numpy as np

from oracle import n2nmn_oracle as O
from n2nmn_amd import synth
from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES

import beam_oracle as B

NAMES = list(CLEVR_MODULE_NAMES)
D_SMALL = Dims(lstm_dim=64, embed_dim_txt=16, embed_dim_nmn=16, T_encoder=7, T_decoder=6, N=3, D=16, map_dim=8)


def _setup(d, seed, n, scale=1.0):
    w = synth.make_weights(d, seed=seed)
    if scale != 1.0:        # sharper token distributions: the search has something to find
        for k in w:
            if 'token_prediction/weights' in k:
                w[k] = w[k] * scale
    batch = synth.make_inputs(d, seed=seed, n=n, min_len=1)
    enc = O.encoder_forward(w, batch['input_seq_batch'], batch['seq_length_batch'], np.float64)
    return w, batch, enc


def test_beam_of_one_is_greedy():
    d = dataclasses.replace(D_SMALL, T_decoder=12)
    P, Wv, bv = O.build_validity_mats(NAMES)
    w, batch, enc = _setup(d, 3, 5, scale=4.0)
    dec = O.decoder_forward(w, enc, P, Wv, bv, d.T_decoder, np.float64)
    bs = B.beam_search(w, enc, P, Wv, bv, d.T_decoder, 1)
    assert np.array_equal(bs['tokens'][0], dec['predicted_tokens'])
    assert np.array_equal(bs['scores'][0], B.seq_log_prob(dec['token_probs']))


def test_wide_beam_finds_the_true_maximum():
    d = D_SMALL
    T = d.T_decoder
    P, Wv, bv = O.build_validity_mats(NAMES)
    layouts, widest = B.all_layouts(P, Wv, bv, T)
    M = layouts.shape[0]
    assert (M, widest) == (1152, 1152)
    n = 3
    w, batch, enc = _setup(d, 7, n, scale=4.0)
    # every layout of every question, one forced-token decoder run: column m * n + i = layout m, question i
    seq = np.tile(batch['input_seq_batch'], (1, M))
    lens = np.tile(batch['seq_length_batch'], M)
    enc_all = O.encoder_forward(w, seq, lens, np.float64)
    forced = np.repeat(layouts.T, n, axis=1)
    dec = O.decoder_forward(w, enc_all, P, Wv, bv, T, np.float64, forced_tokens=forced)
    assert dec['token_validity'][np.arange(T)[:, None], np.arange(M * n)[None, :], forced].all()
    lsp = B.seq_log_prob(dec['token_probs']).reshape(M, n)
    bs = B.beam_search(w, enc, P, Wv, bv, T, widest)
    for i in range(n):
        best = int(np.argmax(lsp[:, i]))
        assert np.array_equal(bs['tokens'][0, :, i], layouts[best]), i
        assert abs(bs['scores'][0, i] - lsp[best, i]) <= 1e-12
        # the beam kept every layout: its scores are all of them, in descending order
        assert np.all(np.diff(bs['scores'][:, i]) <= 0)
        assert np.abs(np.sort(bs['scores'][:, i]) - np.sort(lsp[:, i])).max() <= 1e-12
    # greedy is not always the maximum on these inputs (otherwise the search shows nothing)
    greedy = O.decoder_forward(w, enc, P, Wv, bv, T, np.float64)
    assert (B.seq_log_prob(greedy['token_probs']) <= bs['scores'][0] + 1e-12).all()


def test_every_beam_scores_as_its_forced_decode():
    d = dataclasses.replace(D_SMALL, T_decoder=10)
    P, Wv, bv = O.build_validity_mats(NAMES)
    w, batch, enc = _setup(d, 11, 4, scale=4.0)
    K = 5
    bs = B.beam_search(w, enc, P, Wv, bv, d.T_decoder, K)
    assert np.isfinite(bs['scores']).all()
    for k in range(K):
        dec = O.decoder_forward(w, enc, P, Wv, bv, d.T_decoder, np.float64, forced_tokens=bs['tokens'][k])
        assert dec['token_validity'][np.arange(d.T_decoder)[:, None], np.arange(4)[None, :], bs['tokens'][k]].all()
        assert np.abs(B.seq_log_prob(dec['token_probs']) - bs['scores'][k]).max() <= 1e-12
    assert (np.diff(bs['scores'], axis=0) <= 0).all()
    for i in range(4):          # K distinct layouts per question
        assert len({tuple(bs['tokens'][k, :, i]) for k in range(K)}) == K


def test_latch_on_all_valid_tables():
    d = dataclasses.replace(D_SMALL, T_decoder=7, num_vocab_nmn=5)
    V = d.num_vocab_nmn
    eos = V - 1
    P = np.zeros((V, 3), np.int64); Wv = np.zeros((3, V, 4), np.int64); bv = np.zeros((V, 4), np.int64)
    w, batch, enc = _setup(d, 13, 4, scale=4.0)
    K = 4
    bs = B.beam_search(w, enc, P, Wv, bv, d.T_decoder, K, latch_eos=eos)
    for k in range(K):
        tok = bs['tokens'][k]
        dec = O.decoder_forward(w, enc, P, Wv, bv, d.T_decoder, np.float64, forced_tokens=tok)
        for i in range(4):
            hit = np.nonzero(tok[:, i] == eos)[0]
            upto = d.T_decoder if hit.size == 0 else int(hit[0]) + 1
            assert (tok[upto:, i] == eos).all()
            want = np.log(dec['token_probs'][:upto, i]).sum()
            assert abs(want - bs['scores'][k, i]) <= 1e-12
