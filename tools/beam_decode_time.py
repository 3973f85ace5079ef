"""Cost of beam-search layout decoding (include/n2nmn.h section 2b) at N = 64 questions, CLEVR dimensions:
decode-only (Engine.seq2seq: encoder + decoder) and decode + walk (Engine.forward, nothing fetched) questions/s
for K in {1, 2, 4, 10, 16}, and per K the yardstick -- the GREEDY decoder half at the same number of decoder
rows (N' = K * 64 questions) against the beam decoder half, both over encoder results already in the context
(the whole greedy call at N' would also run a K times larger encoder).  Timed with HIP events around each
call: 5 warm-up calls, 30 timed, median and the 10 % .. 90 % spread.  Every measurement runs in a child process
of its own under a time limit; the first failure ends the run.  Writes profiles/beam_search.md.

    python tools/beam_decode_time.py [--reps 30] [--out profiles/beam_search.md]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
KS = (1, 2, 4, 10, 16)
NQ = 64


def child(K, n, reps):
    import numpy as np
    import torch
    from n2nmn_amd import synth
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
    d = Dims(N=n)
    eng = Engine(d, Assembler(list(CLEVR_MODULE_NAMES)))
    w = synth.make_weights(d, seed=0)
    # token_prediction/weights x 100, as in tests/test_gpu_beam.py: with the flat distributions of random initial
    # weights greedy emits long layouts and a beam the shortest valid one, so their walk times could not be compared
    for k in w:
        if k.endswith('token_prediction/weights'):
            w[k] = (w[k] * np.float32(100.0)).astype(np.float32)
    eng.load_weights(w)
    batch = synth.make_inputs(d, seed=3, n=n)
    dev = {k: torch.as_tensor(v).to(eng.device) for k, v in batch.items()}
    seq, lens = dev['input_seq_batch'], dev['seq_length_batch']

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms = np.sort(np.array(ms))
        return dict(median_ms=float(np.median(ms)), p10_ms=float(ms[len(ms) // 10]), p90_ms=float(ms[-1 - len(ms) // 10]))

    res = dict(K=K, N=n, reps=reps)
    res['decode'] = timed(lambda: eng.seq2seq(seq, lens, beam_size=K, word_vecs=False))
    eng.seq2seq(seq, lens, phase='encoder')        # the decoder half alone, over these encoder results
    res['decoder_only'] = timed(lambda: eng.seq2seq(seq, lens, beam_size=K, word_vecs=False, phase='decoder'))
    res['decode_walk'] = timed(lambda: eng.forward(dev, beam_size=K, fetch=False))
    tok = eng.seq2seq(seq, lens, beam_size=K, word_vecs=False)['predicted_tokens'].cpu().numpy()
    eos = tok == d.num_vocab_nmn - 1
    res['layout_len'] = float(np.where(eos.any(0), eos.argmax(0), tok.shape[0]).mean())
    if K > 1:        # share of the new kernels: the library's per-family event profile of one decoder-half call
        eng.seq2seq(seq, lens, phase='encoder')
        eng.profile_begin()
        eng.seq2seq(seq, lens, beam_size=K, word_vecs=False, phase='decoder')
        res['families'] = {f['name']: [f['launches'], f['total_ms']] for f in eng.profile_end() if f['launches']}
    print('RESULT ' + json.dumps(res), flush=True)


def run_child(K, n, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(K), '--n', str(n), '--reps', str(reps)],
                         capture_output=True, text=True, timeout=240)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
        raise SystemExit('measurement K=%d N=%d failed with status %d: stopping' % (K, n, out.returncode))
    line = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', type=int, default=0)
    ap.add_argument('--n', type=int, default=NQ)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'beam_search.md'))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, max(20, a.reps))
    rows = []
    for K in KS:
        beam = run_child(K, NQ, a.reps)
        yard = run_child(1, K * NQ, a.reps) if K > 1 else beam
        rows.append((K, beam, yard))
        print(K, beam['decode'], beam['decoder_only'], yard['decoder_only'], flush=True)
    with open(a.out, 'w') as f:
        f.write('# Beam-search layout decoding: measured cost\n\n')
        f.write('`python tools/beam_decode_time.py` on one MI355X, CLEVR dimensions (lstm_dim 512, T_enc 45, T_dec 20), '
                'N = 64 questions, seed-0 synthetic weights with token_prediction/weights x 100 (the weights of '
                'tests/test_gpu_beam.py; with them greedy and every beam width choose layouts of the same mean length, '
                'last column, so the decode + walk rows are comparable with each other -- but these are SHORT layouts: '
                'the walk share is a lower bound for trained weights), latency mode, HIP events around each call, 5 warm-up + %d timed calls, median '
                '(10 %% .. 90 %%).  Yardstick: greedy decode (beam_size 1) of K * 64 questions, i.e. the same number of '
                'decoder rows, same tool; the last three columns time the DECODER half alone (phase=\'decoder\' over encoder '
                'results already held), so the yardstick does not carry a K times larger encoder.\n\n' % max(20, a.reps))
        f.write('| K | decode ms | questions/s | decode + walk ms | questions/s | beam decoder half ms | greedy decoder half at 64 K rows ms | beam / yardstick | mean layout length |\n')
        f.write('|---|---|---|---|---|---|---|---|---|\n')
        for K, b, y in rows:
            d_, w_ = b['decode'], b['decode_walk']
            o_, yo = b['decoder_only'], y['decoder_only']
            f.write('| %d | %.3f (%.3f .. %.3f) | %.0f | %.3f (%.3f .. %.3f) | %.0f | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %.1f |\n' % (
                K, d_['median_ms'], d_['p10_ms'], d_['p90_ms'], NQ / d_['median_ms'] * 1e3,
                w_['median_ms'], w_['p10_ms'], w_['p90_ms'], NQ / w_['median_ms'] * 1e3,
                o_['median_ms'], o_['p10_ms'], o_['p90_ms'], yo['median_ms'], yo['p10_ms'], yo['p90_ms'],
                o_['median_ms'] / yo['median_ms'], b['layout_len']))
        f.write('\nPer-family event profile of one beam DECODER-half call (launches, total ms; every entry carries its '
                'event pair, ~4 us, so the shares of the short kernels are upper bounds).  `beam(...)` = 20 select + 19 '
                'gather launches in 20 entries, and the backtrack:\n\n')
        for K, b, _ in rows:
            if 'families' in b:
                tot = sum(v[1] for v in b['families'].values())
                beam_ms = sum(v[1] for k, v in b['families'].items() if k.startswith('beam('))
                f.write('* K = %d: select + gather + backtrack %.3f ms of %.3f ms profiled = %.0f %%  (%s)\n' % (
                    K, beam_ms, tot, 100.0 * beam_ms / tot,
                    ', '.join('%s %d x %.3f ms' % (k, v[0], v[1]) for k, v in b['families'].items())))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
