"""dec_attn_ring_kernel (csrc/kernels_seq2seq.hip): the teacher-forced decoder attention of one question in an
8-wave workgroup with at most 48 KB of LDS, the question's encoder_h_transform rows streamed through a two-slot
ring of 8-row chunks by LDS-DMA.  Every case runs twice on the same context: the launch counter of
n2nmn_debug_dec_attn proves that each run went through the ring kernel, the two runs must return the SAME BITS in
every fetched output (a missed wait in the ring shows as a run that scored rows still in flight), and the outputs
must meet the fp64 oracle at the tolerances of test_gpu_seq2seq.py (util.check_decoder).

Shapes: N = 128 (the smallest launch that reaches the kernel), lstm_dim 512, T_enc 45; question lengths 1,
chunk - 1, chunk, chunk + 1, 2 chunk, 44 and 45 (45: no virtual bias row) plus a seeded random remainder; T_dec 2,
5, 6, 11, 20 (one, two and four step groups of five, full and partly filled); layouts that end after 0, 1, 5, 6
and all steps under eos_retire; and two contexts on two streams at once, one of them with 1024-row encoder steps."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import n2nmn_oracle as O
from n2nmn_amd import _lib, synth
from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
from util import assert_close, check_decoder, t2n

pytestmark = pytest.mark.gpu
N, CHUNK, NBIG = 128, 8, 1024
NAMES = list(CLEVR_MODULE_NAMES)
FETCH = ('predicted_tokens', 'token_probs', 'neg_entropy', 'atts', 'word_vecs', 'log_seq_prob', 'token_scores')


@pytest.fixture(scope='module')
def big():
    """one context of 1024 rows (the concurrent case needs 1024-row encoder steps), seed-0 weights"""
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.engine import Engine
    d = Dims(N=NBIG)
    asm = Assembler(NAMES)
    eng = Engine(d, asm)
    w = synth.make_weights(d, seed=0)
    eng.load_weights(w)
    return eng, d, asm, w


@pytest.fixture(scope='module')
def questions(big):
    """128 questions with the hand-set lengths in front, and their fp64 encoder (computed once, never changed)"""
    eng, d, asm, w = big
    T = d.T_encoder
    batch = synth.make_inputs(d, seed=31, n=N, min_len=1)
    lens = batch['seq_length_batch'].copy()
    edge = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, T - 1, T]
    lens[:len(edge)] = edge
    seq = batch['input_seq_batch'].copy()
    seq[np.arange(T)[:, None] >= lens[None, :]] = 0
    batch = dict(batch, seq_length_batch=lens, input_seq_batch=seq)
    enc = O.encoder_forward(w, seq, lens, np.float64)
    return batch, enc


def _layouts(Td, seed, lengths=None):
    """[Td, N] tokens: `lengths[i]` module tokens, then <eos> (teacher forcing takes any token as valid)"""
    rng = np.random.default_rng(seed)
    eos = len(NAMES) - 1
    k = rng.integers(0, Td + 1, size=N) if lengths is None else np.asarray(lengths)
    gt = rng.integers(0, eos, size=(Td, N)).astype(np.int32)
    gt[np.arange(Td)[:, None] >= k[None, :]] = eos
    return gt, k


def _launches(eng):
    """launches of dec_attn_ring_kernel in this process so far (slot 0 of n2nmn_debug_dec_attn)"""
    out = (ctypes.c_uint64 * 4)()
    _lib.check(eng._lib.n2nmn_debug_dec_attn(eng._ctx, out))
    return int(out[0])


def _same_bits(what, a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), '%s: %s differs between two runs (max |diff| %.3e)' % (
            what, k, float(np.max(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)))))


def _twice(what, eng, run):
    """run() twice on the same context: each run launched the ring kernel at least once, and the two returned the
    same bits in every fetched output; the first run's outputs"""
    got = []
    for i in range(2):
        before = _launches(eng)
        got.append(run())
        assert _launches(eng) - before >= 1, '%s: run %d did not launch dec_attn_ring_kernel' % (what, i)
    _same_bits(what, got[0], got[1])
    return got[0]


@pytest.mark.parametrize('Td', [2, 5, 6, 11, 20])
def test_ring_kernel_meets_the_oracle_and_repeats_bit_for_bit(big, questions, Td):
    eng, d, asm, w = big
    batch, enc = questions
    gt, _ = _layouts(Td, seed=Td)

    def run():
        out = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], T_dec=Td, use_gt_layout=True,
                          gt_layout=gt, debug=True, reuse_buffers=False)
        torch.cuda.synchronize()
        return {k: t2n(out[k]).copy() for k in FETCH}

    ring = _twice('T_dec %d' % Td, eng, run)
    assert np.array_equal(ring['predicted_tokens'], gt)
    dec = O.decoder_forward(w, enc, asm.P, asm.W, asm.b, Td, np.float64, use_gt_layout=True, gt_layout=gt)
    diffs = check_decoder(ring, dec)
    print('T_dec %2d vs fp64: %s' % (Td, ', '.join('%s %.2e' % kv for kv in diffs.items())))
    # rows past a question's length carry no weight, the others sum to 1 (the virtual bias row stands for all
    # of the former: its score is copied, then masked)
    lens = batch['seq_length_batch']
    past = np.arange(d.T_encoder)[None, :, None] >= lens[None, None, :]
    assert np.all(ring['atts'][np.broadcast_to(past, ring['atts'].shape)] == 0.0)
    assert np.abs(ring['atts'].sum(axis=1) - 1.0).max() < 1e-5


def test_unknown_setting_is_refused_and_the_retired_key_with_it(big):
    eng = big[0]
    for key in ('dec_attn_ring', 'dec_attn_rings'):
        with pytest.raises(KeyError):
            eng.debug_set(key, 1)


def test_logits_tokens_and_validity_of_a_whole_pass(big, questions):
    """decoder -> layout walker: scores, tokens and validity of Engine.forward, scores against the fp64 oracle"""
    eng, d, asm, w = big
    batch, enc = questions
    gt = synth.template_layout_batch(d, n=N, offset=3)

    def run():
        sc, tok, val = eng.forward(batch, use_gt_layout=True, gt_layout=gt)
        return dict(scores=t2n(sc).copy(), tokens=np.asarray(tok).copy(), validity=np.asarray(val).copy())

    ring = _twice('forward', eng, run)
    assert np.array_equal(ring['tokens'], gt) and ring['validity'].all()
    # O.forward's stages on the shared fp64 encoder; bar and helper of test_gpu_end2end.py
    dec = O.decoder_forward(w, enc, asm.P, asm.W, asm.b, d.T_decoder, np.float64, use_gt_layout=True, gt_layout=gt)
    exprs, validity = O.assemble(NAMES, dec['predicted_tokens'])
    assert validity.all()
    ref = O.execute_layouts(w, exprs, batch['image_feat_batch'], dec['word_vecs'], d.num_choices, np.float64)
    assert_close('scores', ring['scores'], ref, 1e-4)


def test_layouts_that_end_early_under_eos_retire(big, questions):
    """dec_len 0, 1, 5, 6 and all 20 steps (the step-group thresholds of the kernel: <= 5 steps give every wave to
    the rows, <= 10 half of them) plus a random remainder; the dead steps are not written at all"""
    eng, d, asm, w = big
    batch, enc = questions
    Td = d.T_decoder
    k = np.random.default_rng(5).integers(0, Td + 1, size=N)
    k[:10] = [0, 1, 5, 6, Td, Td, 6, 5, 1, 0]
    gt, k = _layouts(Td, seed=77, lengths=k)
    keys = ('predicted_tokens', 'token_probs', 'atts', 'word_vecs')

    def run():
        for key, shape, dt in (('tp', (Td, N), torch.float32), ('att', (Td, d.T_encoder, N), torch.float32),
                               ('wv', (Td, N, d.embed_dim_txt), torch.float32)):
            eng._buf(key, shape, dt).zero_()
        out = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], use_gt_layout=True, gt_layout=gt,
                          eos_retire=True, gt_len_host=k.astype(np.int32))
        torch.cuda.synchronize()
        return {key: t2n(out[key]).copy() for key in keys if key in out}

    eng.set_mode('throughput')
    try:
        ring = _twice('eos_retire', eng, run)
    finally:
        eng.set_mode('latency')
    assert np.array_equal(ring['predicted_tokens'], gt)
    live = np.arange(Td)[:, None] < k[None, :]                          # [Td, N]
    dead_att = ring['atts'][np.broadcast_to(~live[:, None, :], ring['atts'].shape)]
    assert np.all(dead_att == 0.0), 'a retired step was evaluated: the case does not exercise dec_len'
    dec = O.decoder_forward(w, enc, asm.P, asm.W, asm.b, Td, np.float64, use_gt_layout=True, gt_layout=gt)
    ref_att = np.where(live[:, None, :], dec['atts'][..., 0], 0.0)
    assert_close('atts of the live steps', ring['atts'], ref_att, 1e-4)
    assert_close('token_probs of the live steps', np.where(live, ring['token_probs'], 0.0),
                 np.where(live, dec['token_probs'], 0.0), 1e-4)


def test_context_vectors_of_a_training_forward(questions):
    """the context vectors only the backward pass reads (n2nmn_train_debug_tensor "dec_ctx") and the recorded
    token logits: same bits in two runs, and ctx = sum_tau att[tau] encoder_outputs[tau] of the oracle"""
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.train import Trainer
    batch, enc = questions
    d = Dims(N=N)
    asm = Assembler(NAMES)
    eng = Engine(d, asm)
    w = synth.make_weights(d, seed=0)
    eng.load_weights(w)
    tr = Trainer(eng)
    gt = synth.template_layout_batch(d, n=N, offset=1)
    Td, L = d.T_decoder, d.lstm_dim

    def run():
        tr.forward_backward(batch, gt, reduce=False)
        out = dict(dec_ctx=t2n(tr.debug_tensor('dec_ctx', (Td, N, L))).copy(),
                   token_scores=t2n(tr.debug_tensor('token_scores', (Td, N, d.num_vocab_nmn))).copy())
        torch.cuda.synchronize()
        return out

    ring = _twice('training forward', eng, run)
    dec = O.decoder_forward(w, enc, asm.P, asm.W, asm.b, Td, np.float64, use_gt_layout=True, gt_layout=gt)
    ctx = np.einsum('jtn,tnl->jnl', dec['atts'][..., 0], enc['outputs'])
    assert_close('dec_ctx', ring['dec_ctx'], ctx, 1e-4)
    assert_close('token_scores', ring['token_scores'], dec['token_scores'], 1e-4)


def test_two_contexts_on_two_streams_equal_the_passes_run_alone(big, questions):
    """context A: passes of 1024 questions (1024-row encoder steps on the recurrent tile kernel, then its
    decoder); context B (a fork): passes of the 128 questions above, on a second stream at the same time, so the
    attention workgroups of one meet the tile and attention workgroups of the other on the same CUs.  One round, no
    soak loop: the round queues two passes on A's stream and four short ones on B's only so that the two streams
    stay busy side by side for the length of A's passes (a single B pass ends before A's decoder begins); each
    result must be the bits of the same pass run alone."""
    eng, d, asm, w = big
    batch, _ = questions
    fork = eng.fork()
    dev = eng.device
    bigb = synth.make_inputs(d, seed=32, n=NBIG, min_len=1)
    gtA = torch.as_tensor(synth.clevr_like_layout_batch(d, n=NBIG, seed=3)).to(dev)
    gtB = torch.as_tensor(synth.template_layout_batch(d, n=N, offset=5)).to(dev)
    inA = [torch.as_tensor(bigb[k]).to(dev) for k in ('input_seq_batch', 'seq_length_batch')]
    inB = [torch.as_tensor(batch[k]).to(dev) for k in ('input_seq_batch', 'seq_length_batch')]
    keys = ('predicted_tokens', 'token_probs', 'neg_entropy', 'atts', 'word_vecs', 'log_seq_prob')

    def one(e, ins, gt):
        return e.seq2seq(ins[0], ins[1], use_gt_layout=True, gt_layout=gt, reuse_buffers=False)

    def host(out):
        return {k: t2n(out[k]).copy() for k in keys}

    for e in (eng, fork):
        e.set_mode('throughput')
    try:
        torch.cuda.synchronize()
        aloneA = host(one(eng, inA, gtA))
        torch.cuda.synchronize()
        aloneB = host(one(fork, inB, gtB))
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        with torch.cuda.stream(sa):
            outA = [one(eng, inA, gtA) for _ in range(2)]
        with torch.cuda.stream(sb):
            outB = [one(fork, inB, gtB) for _ in range(4)]
        torch.cuda.synchronize()
        for o in outA:
            _same_bits('1024-row context, concurrent vs alone', host(o), aloneA)
        for o in outB:
            _same_bits('128-row context, concurrent vs alone', host(o), aloneB)
    finally:
        for e in (eng, fork):
            e.set_mode('latency')
