"""E of tests/test_gpu_beam.py: on that file's inputs, max over all cases and beams of
|log_seq_prob(GPU decoder forced to the oracle's tokens) - fp64 oracle score| -- the existing fp32 decoder
against fp64, nothing of the beam code.  The test's margin is 4 E, its score tolerance 2 E.

    python tools/beam_forced_error.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    import test_gpu_beam as T
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import Dims
    eng = Engine(Dims(N=256), Assembler(T.NAMES))
    eng.load_weights(T.clevr_weights())
    worst = 0.0
    for K, N in T.CASES:
        batch, bs = T.oracle_case(K, N)
        e = 0.0
        for k in range(K):
            live = np.isfinite(bs['scores'][k])
            f = T._forced(eng, batch, bs['tokens'][k])
            if live.any():
                e = max(e, float(np.abs(f['log_seq_prob'] - bs['scores'][k])[live].max()))
        worst = max(worst, e)
        print('K %2d N %3d: E = %.3e   smallest oracle gap %.3e' % (K, N, e, bs['min_gap'].min()), flush=True)
    print('E = %.3e  ->  margin 4 E = %.3e, score tolerance 2 E = %.3e' % (worst, 4 * worst, 2 * worst))
    und = sum(int((T.oracle_case(K, N)[1]['min_gap'] < 4 * worst).sum()) for K, N in T.CASES)
    print('undecidable (question, K) cases at that margin: %d / %d' % (und, sum(N for _, N in T.CASES)))
    # the two other dimension sets of the test file reuse that margin: their own E must not exceed it
    import beam_oracle as B
    eng, d, w, Z, batch, enc = T.shapes_setup()
    e = 0.0
    for K in (2, 5):
        bs = B.beam_search(w, enc, Z[0], Z[1], Z[2], d.T_decoder, K, latch_eos=d.num_vocab_nmn - 1)
        for k in range(K):
            tok = bs['tokens'][k]
            f = eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], d.T_decoder, forced_tokens=tok,
                            reuse_buffers=False)
            # (the greedy call has no latch: count the steps up to and including a beam's first <eos>)
            seen = np.cumsum(tok == d.num_vocab_nmn - 1, axis=0) > 0
            behind = np.vstack([np.zeros((1, tok.shape[1]), bool), seen[:-1]])
            lsp = np.where(behind, 0.0, np.log(f['token_probs'].cpu().numpy().astype(np.float64))).sum(0)
            e = max(e, float(np.abs(lsp - bs['scores'][k]).max()))
    print('models_shapes dimensions (lstm_dim 256, latch): E = %.3e' % e)
    eng, d, w, seq, lens, enc = T.vqa_setup()
    asm = eng.assembler
    bs = B.beam_search(w, enc, np.asarray(asm.P), np.asarray(asm.W), np.asarray(asm.b), d.T_decoder, 4)
    e = 0.0
    for k in range(4):
        f = eng.engine.seq2seq(seq, lens, d.T_decoder, forced_tokens=bs['tokens'][k], reuse_buffers=False)
        live = np.isfinite(bs['scores'][k])
        e = max(e, float(np.abs(f['log_seq_prob'].cpu().numpy() - bs['scores'][k])[live].max()))
    print('models_vqa dimensions (lstm_dim 1000): E = %.3e' % e)


if __name__ == '__main__':
    main()
