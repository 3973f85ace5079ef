"""Beam-search layout decoding on the device (include/n2nmn.h section 2b; Engine.seq2seq(beam_size=K)) against
the fp64 beam search of tests/beam_oracle.py (pinned on the CPU by tests/test_beam_oracle_host.py).

Inputs: CLEVR dimensions, seed-0 synthetic weights with token_prediction/weights scaled by TOKEN_SCALE (random
initial logits are nearly flat: the K best prefixes would sit within 1e-3 of each other and nothing could be
compared), questions of mixed lengths including 1 and T_encoder.

Tolerances come from a measurement of the EXISTING fp32 decoder, nothing of the new code: on these inputs,
E = max over all cases and beams of |log_seq_prob(GPU, forced to the oracle's tokens) - oracle score|
(tools/beam_forced_error.py).  Measured on an MI355X: E = 3.875e-05 (K = 16, N = 64; 2.7e-05 .. 3.9e-05 at
N >= 7, ~1e-05 at N = 1), so the decision margin is m = 4 E = 1.55e-04 (2 x for two scores being compared, 2 x
headroom) and the score tolerance 2 E = 7.75e-05; 2 of the 544 (question, K) cases are undecidable at that m
(both at K = 4, N = 256), and the largest |score - oracle| the beam decoder returned was 3.87e-05.
A question is decidable for a K iff no decision of the oracle's search (K-th candidate against the first one dropped at any step; adjacent
ranks of the final order) has a gap below m.  At most 2 % of the (question, K) cases may be undecidable
(asserted); undecidable questions must still return an accepted layout whose score is its own forced score.
"""
import functools

import numpy as np
import pytest

from oracle import n2nmn_oracle as O
from n2nmn_amd import synth
from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
from util import assert_close, t2n

import beam_oracle as B

pytestmark = pytest.mark.gpu
NAMES = list(CLEVR_MODULE_NAMES)
TOKEN_SCALE = 100.0
E_FORCED = 3.875e-5        # measured (tools/beam_forced_error.py), see above
MARGIN = 4 * E_FORCED
SCORE_TOL = 2 * E_FORCED
CASES = [(K, N) for K in (2, 4, 10, 16) for N in (1, 7, 64)] + [(4, 256)]


def scaled_weights(w, scale=TOKEN_SCALE):
    w = dict(w)
    for k in w:
        if k.endswith('token_prediction/weights'):
            w[k] = (w[k] * np.float32(scale)).astype(np.float32)
    return w


@functools.lru_cache(maxsize=None)
def clevr_weights():
    return scaled_weights(synth.make_weights(Dims(), seed=0))


def make_batch(d, n, seed):
    batch = synth.make_inputs(d, seed=seed, n=n, min_len=1)
    lens = batch['seq_length_batch'].copy()
    lens[0] = 1 if seed % 2 else d.T_encoder          # the extremes are always there
    if n > 1:
        lens[1] = d.T_encoder if seed % 2 else 1
    seq = batch['input_seq_batch'].copy()
    seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
    return dict(batch, seq_length_batch=lens, input_seq_batch=seq)


@functools.lru_cache(maxsize=None)
def oracle_case(K, N):
    d = Dims()
    P, Wv, bv = O.build_validity_mats(NAMES)
    batch = make_batch(d, N, 100 * K + N)
    enc = O.encoder_forward(clevr_weights(), batch['input_seq_batch'], batch['seq_length_batch'], np.float64)
    return batch, B.beam_search(clevr_weights(), enc, P, Wv, bv, d.T_decoder, K)


@pytest.fixture(scope='module')
def beam_engine():
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    d = Dims(N=256)
    asm = Assembler(NAMES)
    eng = Engine(d, asm)
    eng.load_weights(clevr_weights())
    return eng, d, asm


def _beam(eng, batch, K, **kw):
    out = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], beam_size=K, return_beams=True,
                      reuse_buffers=False, **kw)
    return {k: t2n(v) for k, v in out.items() if not k.startswith('_')}


def _forced(eng, batch, tokens):
    out = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], forced_tokens=tokens,
                      reuse_buffers=False)
    return {k: t2n(v) for k, v in out.items() if not k.startswith('_')}


def test_beam_size_one_is_the_greedy_call(beam_engine):
    eng, d, asm = beam_engine
    batch = make_batch(d, 64, 5)
    a = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], reuse_buffers=False)
    b = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], reuse_buffers=False, beam_size=1)
    for k in ('predicted_tokens', 'token_probs', 'atts', 'word_vecs', 'log_seq_prob', 'neg_entropy'):
        assert np.array_equal(t2n(a[k]), t2n(b[k])), k


@pytest.mark.parametrize('K,N', CASES)
def test_beams_equal_the_oracle(beam_engine, K, N):
    eng, d, asm = beam_engine
    batch, bs = oracle_case(K, N)
    got = _beam(eng, batch, K)
    ok = bs['min_gap'] >= MARGIN
    print('K %d N %d: decidable %d / %d, smallest gap %.3e' % (K, N, ok.sum(), N, bs['min_gap'].min()))
    assert np.array_equal(got['predicted_tokens'], got['beam_tokens'][0])
    assert np.array_equal(got['beam_tokens'][:, :, ok], bs['tokens'][:, :, ok])
    live = np.isfinite(bs['scores'])
    assert np.array_equal(np.isfinite(got['beam_scores'])[:, ok], live[:, ok])
    diff = np.abs(np.where(live, got['beam_scores'] - bs['scores'], 0.0))[:, ok]
    print('  max |score - oracle| = %.3e' % (diff.max() if diff.size else 0.0))
    assert (diff <= SCORE_TOL).all()
    assert_close('log_seq_prob vs beam_scores[0]', got['log_seq_prob'], got['beam_scores'][0], 1e-5)
    # every question, decidable or not: an accepted layout whose score is the forced score of its own tokens
    _, validity = asm.assemble_packed(got['predicted_tokens'])
    assert validity.all()
    f = _forced(eng, batch, got['predicted_tokens'])
    assert np.array_equal(f['predicted_tokens'], got['predicted_tokens'])
    assert_close('own forced score', f['log_seq_prob'], got['beam_scores'][0], SCORE_TOL)
    assert (np.diff(got['beam_scores'], axis=0) <= 0).all()          # the final order


@pytest.mark.parametrize('Td', [3, 4])
def test_tie_order_is_the_headers(beam_engine, Td):
    """Where the order of EQUAL candidates shows.  With T_dec = 3 the CLEVR automaton accepts 6 layouts (40 at
    T_dec = 4), so at K = 16 most candidates of the first steps are -inf and tie: the header orders them by beam,
    then token.  At T_dec = 3 ten dead beams reach the final order -- their tokens and their -inf scores are
    the tie-break's; at T_dec = 4 all 16 final beams are live and the tie-break shows in beam_parents (which
    beam of step t a beam extends).  Compared on the questions whose finite candidates are >= m apart at every
    rank of every step (gap_order), where the names of the beams are decided too."""
    eng, d, asm = beam_engine
    K, N = 16, 7
    P, Wv, bv = O.build_validity_mats(NAMES)
    batch = make_batch(d, N, 500 + Td)
    enc = O.encoder_forward(clevr_weights(), batch['input_seq_batch'], batch['seq_length_batch'], np.float64)
    bs = B.beam_search(clevr_weights(), enc, P, Wv, bv, Td, K)
    got = _beam(eng, batch, K, T_dec=Td)
    ok = bs['gap_order'] >= MARGIN
    dead = np.isinf(bs['scores'])
    print('T_dec %d: comparable %d / %d, dead final beams per question %s' % (Td, ok.sum(), N, dead.sum(0)))
    assert (~ok).sum() <= 0.02 * N                      # (none: 7 questions)
    assert dead.any() == (Td == 3)
    assert got['beam_parents'].shape == (Td, K, N) and got['beam_parents'].min() >= 0 and got['beam_parents'].max() < K
    assert np.array_equal(got['beam_parents'][:, :, ok], bs['parents'][:, :, ok])
    assert np.array_equal(got['beam_tokens'][:, :, ok], bs['tokens'][:, :, ok])           # dead beams included
    assert np.array_equal(np.isinf(got['beam_scores'])[:, ok], dead[:, ok])
    with np.errstate(invalid='ignore'):                  # (-inf - -inf of the dead beams, masked out)
        diff = np.where(dead, 0.0, got['beam_scores'] - bs['scores'])
    assert (np.abs(diff)[:, ok] <= SCORE_TOL).all()
    _, validity = asm.assemble_packed(got['predicted_tokens'])
    assert validity.all()


def test_parents_of_the_long_cases(beam_engine):
    """beam_parents against the oracle at T_dec = 20 (K = 10, N = 7), on the questions whose order is decided at
    every rank of every step; the first steps have dead beams, so the tie-break is part of it"""
    eng, d, asm = beam_engine
    batch, bs = oracle_case(10, 7)
    got = _beam(eng, batch, 10)
    ok = bs['gap_order'] >= MARGIN
    print('parents: comparable %d / 7' % ok.sum())
    assert ok.any()
    assert np.array_equal(got['beam_parents'][:, :, ok], bs['parents'][:, :, ok])


def test_faces_pass_beam_size(beam_engine):
    """the reference-named faces hand beam_size= to the engine: AttentionSeq2Seq.run equals Engine.seq2seq"""
    from n2nmn_amd.nmn3_netgen_att import AttentionSeq2Seq
    from n2nmn_amd.nmn3_model import NMN3Model
    eng, d, asm = beam_engine
    batch, _ = oracle_case(4, 7)
    seq, lens = batch['input_seq_batch'], batch['seq_length_batch']
    want = _beam(eng, batch, 4)
    args = (seq, lens, d.T_decoder, d.num_vocab_txt, d.embed_dim_txt, d.num_vocab_nmn, d.embed_dim_nmn,
            d.lstm_dim, d.num_layers, asm, False, False, False)
    face = AttentionSeq2Seq(*args, engine=eng, beam_size=4)
    out = face.run()
    for k in ('predicted_tokens', 'token_probs', 'atts', 'word_vecs', 'log_seq_prob'):
        assert np.array_equal(t2n(out[k]).copy(), want[k]), k
    greedy = AttentionSeq2Seq(*args, engine=eng).run()          # the default is the reference's decoding
    g = eng.seq2seq(seq, lens, reuse_buffers=False)
    assert np.array_equal(t2n(greedy['predicted_tokens']).copy(), t2n(g['predicted_tokens']))
    feat = batch['image_feat_batch']
    model = NMN3Model(feat, seq, lens, d.T_decoder, d.num_vocab_txt, d.embed_dim_txt, d.num_vocab_nmn,
                      d.embed_dim_nmn, d.lstm_dim, d.num_layers, asm, False, False, False, d.num_choices,
                      engine=eng, beam_size=4)
    assert np.array_equal(t2n(model.run_phase1()['predicted_tokens']).copy(), want['predicted_tokens'])


def test_shapes_face_passes_beam_size():
    """models_shapes' NMN3ModelAtt(beam_size=): its host-side <eos> latch leaves device-latched beams as they are"""
    from n2nmn_amd.models_shapes import NMN3ModelAtt
    eng, d, w, Z, batch, enc = shapes_setup()
    want = _beam(eng, batch, 3, T_dec=d.T_decoder)
    imgs = np.zeros((64, 30, 30, 3), np.float32)
    face = NMN3ModelAtt(imgs, batch['input_seq_batch'], batch['seq_length_batch'], d.T_decoder, d.num_vocab_txt,
                        d.embed_dim_txt, d.num_vocab_nmn, d.embed_dim_nmn, d.lstm_dim, d.num_layers,
                        d.num_vocab_nmn - 1, False, False, False, d.num_choices, engine=eng, beam_size=3)
    face._cnn = {'conv_1/weights': np.zeros((10, 10, 3, 64), np.float32), 'conv_1/biases': np.zeros(64, np.float32),
                 'conv_2/weights': np.zeros((1, 1, 64, d.D), np.float32), 'conv_2/biases': np.zeros(d.D, np.float32)}
    tok = np.asarray(face.run_phase1()['predicted_tokens'])
    assert np.array_equal(tok, want['predicted_tokens'])         # (the face's own latch had nothing left to change)
    seen = np.cumsum(tok == face.EOS_idx, axis=0) > 0
    assert (tok[1:][seen[:-1]] == face.EOS_idx).all()


def test_undecidable_share(beam_engine):
    und = tot = 0
    for K, N in CASES:
        _, bs = oracle_case(K, N)
        und += int((bs['min_gap'] < MARGIN).sum()); tot += N
    print('undecidable (question, K) cases at m = %.1e: %d / %d' % (MARGIN, und, tot))
    assert und <= 0.02 * tot, (und, tot)


def test_best_beam_is_self_consistent(beam_engine):
    """the existing path forced to the returned best beam reproduces what the search reported (other row
    positions, so not bit for bit): tolerance of tests/test_gpu_lstm_routes.py for these tensors"""
    eng, d, asm = beam_engine
    batch, _ = oracle_case(4, 64)
    got = _beam(eng, batch, 4)
    f = _forced(eng, batch, got['predicted_tokens'])
    for k in ('token_probs', 'atts', 'word_vecs', 'log_seq_prob'):
        assert_close(k, got[k], f[k], 2e-5)
    assert_close('neg_entropy', got['neg_entropy'], f['neg_entropy'], 2e-5)


def test_rows_are_independent(beam_engine):
    eng, d, asm = beam_engine
    K = 4
    batch, _ = oracle_case(K, 64)
    full = _beam(eng, batch, K)
    keys = ('beam_tokens', 'beam_scores', 'predicted_tokens', 'token_probs', 'atts', 'word_vecs', 'log_seq_prob')
    axis = dict(beam_tokens=2, beam_scores=1, predicted_tokens=1, token_probs=1, atts=2, word_vecs=1, log_seq_prob=0)
    perm = np.random.default_rng(3).permutation(64)
    pb = dict(batch, input_seq_batch=np.ascontiguousarray(batch['input_seq_batch'][:, perm]),
              seq_length_batch=np.ascontiguousarray(batch['seq_length_batch'][perm]))
    shuffled = _beam(eng, pb, K)
    for k in keys:
        assert np.array_equal(np.take(full[k], perm, axis=axis[k]), shuffled[k]), k
    for i in (0, 1, 37):
        one = dict(batch, input_seq_batch=np.ascontiguousarray(batch['input_seq_batch'][:, i:i + 1]),
                   seq_length_batch=np.ascontiguousarray(batch['seq_length_batch'][i:i + 1]))
        alone = _beam(eng, one, K)
        for k in keys:
            assert np.array_equal(np.take(full[k], [i], axis=axis[k]), alone[k]), (k, i)


def shapes_setup():
    """models_shapes dimensions on a CLEVR-variant context with all-valid tables (what its inference face builds)"""
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from oracle import n2nmn_oracle_shapes as S
    d = Dims(H=3, W=3, D=64, map_dim=500, lstm_dim=256, num_vocab_txt=14, num_vocab_nmn=5, num_choices=2,
             T_encoder=15, T_decoder=7, N=64, kernel_size=3)
    V = 5
    asm = Assembler(list(S.SHAPES_MODULE_NAMES), op_code={'_Find': 1, '_Transform': 4, '_And': 5, '_Answer': 7},
                    input_num=S.ARITY, output_type=S.OUT_TYPE)
    eng = Engine(d, asm)
    Z = (np.zeros((V, 3), np.int32), np.zeros((3, V, 4), np.int32), np.zeros((V, 4), np.int32))
    eng.set_validity_tables(*Z)
    w = scaled_weights(synth.make_weights(d, seed=2), 30.0)
    eng.load_weights(w)
    batch = make_batch(d, 64, 9)
    enc = O.encoder_forward(w, batch['input_seq_batch'], batch['seq_length_batch'], np.float64)
    return eng, d, w, Z, batch, enc


def vqa_setup():
    from n2nmn_amd import vqa
    d = vqa.VQADims(N=128)
    eng = vqa.VQAEngine(d)
    w = scaled_weights(synth.make_weights_from_shapes(vqa.vqa_variable_shapes(d), seed=0), 30.0)
    eng.load_weights(w)
    rng = np.random.default_rng(17)
    lens = rng.integers(1, d.T_encoder + 1, size=d.N).astype(np.int32)
    lens[:2] = (1, d.T_encoder)
    seq = rng.integers(0, d.num_vocab_txt, size=(d.T_encoder, d.N)).astype(np.int32)
    seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
    enc = O.encoder_forward(w, seq, lens, np.float64)
    return eng, d, w, seq, lens, enc


def test_latch_on_all_valid_tables_and_refusal_without_it():
    """models_shapes dimensions (lstm_dim 256: the general attention kernel), no automaton: <eos> latch per beam.
    Margin and tolerance as above (E on these inputs measured 5.5e-06, below the CLEVR figure); the 2 % limit on
    undecidable questions holds here per case."""
    eng, d, w, Z, batch, enc = shapes_setup()
    eos = d.num_vocab_nmn - 1
    for K in (2, 5):
        bs = B.beam_search(w, enc, Z[0], Z[1], Z[2], d.T_decoder, K, latch_eos=eos)
        got = _beam(eng, batch, K, T_dec=d.T_decoder)
        tok = got['beam_tokens']
        seen = np.cumsum(tok == eos, axis=1) > 0
        assert (tok[:, 1:, :][seen[:, :-1, :]] == eos).all()          # <eos> behind the first <eos>
        ok = bs['min_gap'] >= MARGIN
        print('latch K %d: decidable %d / 64' % (K, ok.sum()))
        assert (~ok).sum() <= 0.02 * ok.size
        assert np.array_equal(tok[:, :, ok], bs['tokens'][:, :, ok])
        assert (np.abs(got['beam_scores'] - bs['scores'])[:, ok] <= SCORE_TOL).all()
    # tables that neither force <eos> nor are all-valid: refused
    Wn = Z[1].copy(); Wn[2, :, 0] = 1                                  # "T_remain >= 0": always true, but a rule
    eng.set_validity_tables(Z[0], Wn, Z[2])
    with pytest.raises(ValueError, match='seq2seq_beam'):
        eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], T_dec=d.T_decoder, beam_size=2)


def test_vqa_dimensions():
    """lstm_dim 1000 (padded to 1024 on the device), 128 questions, K = 4: tokens on decidable rows.  Margin as
    above (E on these inputs measured 4.4e-06, below the CLEVR figure); at most 2 % undecidable."""
    eng, d, w, seq, lens, enc = vqa_setup()
    asm = eng.assembler
    K = 4
    bs = B.beam_search(w, enc, np.asarray(asm.P), np.asarray(asm.W), np.asarray(asm.b), d.T_decoder, K)
    out = eng.engine.seq2seq(seq, lens, d.T_decoder, beam_size=K, return_beams=True, reuse_buffers=False)
    tok = t2n(out['beam_tokens'])
    ok = bs['min_gap'] >= MARGIN
    print('vqa: decidable %d / %d' % (ok.sum(), d.N))
    assert (~ok).sum() <= 0.02 * ok.size
    live = np.isfinite(bs['scores'])
    assert (np.abs(np.where(live, t2n(out['beam_scores']) - bs['scores'], 0.0))[:, ok] <= SCORE_TOL).all()
    assert np.array_equal(tok[:, :, ok], bs['tokens'][:, :, ok])
    assert np.array_equal(t2n(out['predicted_tokens']), tok[0])
    _, validity = asm.assemble_packed(tok[0])
    assert validity.all()


def test_forward_with_beam_and_refused_combinations(beam_engine):
    eng, d, asm = beam_engine
    n = 16
    batch = make_batch(d, n, 77)
    scores, tokens, validity = eng.forward(batch, beam_size=4)
    assert validity.all()
    got = t2n(scores).copy() if hasattr(scores, 'detach') else np.asarray(scores)
    ref = O.forward(clevr_weights(), NAMES, batch, d.T_decoder, d.num_choices, np.float64, use_gt_layout=True,
                    gt_layout=tokens)
    assert_close('scores', got, ref['scores'], 1e-4)
    seq, lens = batch['input_seq_batch'], batch['seq_length_batch']
    with pytest.raises(ValueError, match='beam_size must be'):
        eng.seq2seq(seq, lens, beam_size=17)
    big = make_batch(d, 65, 78)
    with pytest.raises(ValueError, match='1024'):
        eng.seq2seq(big['input_seq_batch'], big['seq_length_batch'], beam_size=16)
    uni = np.random.default_rng(1).random((d.T_decoder, n)).astype(np.float32)
    with pytest.raises(ValueError, match='sample_uniforms'):
        eng.seq2seq(seq, lens, sample_uniforms=uni, beam_size=4)
    with pytest.raises(ValueError, match='EOS_RETIRE'):
        eng.forward(batch, beam_size=4, eos_retire=True)
    with pytest.raises(ValueError, match='forced_tokens'):
        eng.seq2seq(seq, lens, forced_tokens=tokens, beam_size=4)
