"""Cost of VGG-16 pool5 feature extraction (include/n2nmn.h section 9) at 320 x 480, N = 1 and N = 8 images:
ms per image of VGGPool5.forward (HIP events around each call: 3 warm-up calls, `--reps` timed, median and the
10 % .. 90 % spread) and, per layer, the mean time of one launch (n2nmn_vgg_debug_replay: 3 warm-up + 20 launches
of that layer's kernel inside one event pair), its TFLOP/s -- the algorithm's 2 M Cout 9 Cin operations over that
time -- and the fraction of the 157.3 TFLOP/s fp32 MFMA peak.  Beside each convolution from conv1_2 on: the
yardstick, the dense GEMM n2nmn_debug_gemm at the same M = N H W, N = Cout, K = 9 Cin (existing code; timed as
the difference between a call that launches 12 times and one that launches 2, so the pack and the allocation
inside the call cancel; median of 3), and conv / yardstick as a ratio of rates.  conv1_1 and the pools move
bytes: they are reported in GB/s of the bytes they must read and write.  Every measurement runs in a child process of its own under
a time limit; the first failure ends the run.  Writes profiles/vgg_pool5.md.

    python tools/vgg_pool5_time.py [--reps 10] [--out profiles/vgg_pool5.md] [--run-label TEXT]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
H, W = 320, 480
PEAK_TFLOPS = 157.3
NS = (1, 8)


def layer_table(N):
    """name, kind, M, Cin, Cout, flop, bytes (read + write of the dense activation; weights for convs)"""
    from n2nmn_amd import vgg_net
    rows, h, w, cin = [], H, W, 3
    for name in vgg_net.LAYERS:
        if name.startswith('conv'):
            cout = dict((n.split('/')[0], s[3]) for n, s in vgg_net.variable_shapes() if n.endswith('weights'))[name]
            M = N * h * w
            rows.append(dict(name=name, kind='conv', M=M, Cin=cin, Cout=cout, flop=2.0 * M * cout * 9 * cin,
                             bytes=4.0 * (M * cin + M * cout + 9 * cin * cout)))
            cin = cout
        else:
            ho, wo = (h + 1) // 2, (w + 1) // 2
            rows.append(dict(name=name, kind='pool', M=N * ho * wo, Cin=cin, Cout=cin, flop=0.0,
                             bytes=4.0 * (N * h * w * cin + N * ho * wo * cin)))
            h, w = ho, wo
    rows[0]['bytes'] = N * H * W * 3 + 4.0 * (N * H * W * 64 + 27 * 64)        # uint8 input
    return rows


def child(N, reps):
    import numpy as np
    import torch
    from n2nmn_amd import vgg_net
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
    vgg = vgg_net.VGGPool5(max_N=N, max_H=H, max_W=W)
    vgg.load_weights(vgg_net.synthetic_weights(0))
    im = torch.as_tensor(np.random.RandomState(1).randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)).cuda()
    for _ in range(3):
        vgg.forward(im)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); vgg.forward(im); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.sort(np.array(ms))
    res = dict(N=N, reps=reps, median_ms=float(np.median(ms)), p10_ms=float(ms[len(ms) // 10]),
               p90_ms=float(ms[-1 - len(ms) // 10]), layers=[])
    eng = Engine(Dims(), Assembler(list(CLEVR_MODULE_NAMES)))

    def gemm_ms(A, B, bias, launches):
        eng.debug_set('debug_gemm_b3', -launches)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); eng.gemm(A, B, bias); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for L in layer_table(N):
        row = dict(L, us=vgg.replay_us(L['name'], 20) if L['name'] != 'conv1_1' else None)
        if L['kind'] == 'conv' and L['Cin'] != 3:
            K = 9 * L['Cin']
            A = torch.randn((L['M'], K), dtype=torch.float32, device='cuda')
            B = torch.randn((K, L['Cout']), dtype=torch.float32, device='cuda') * 0.01
            bias = torch.zeros((L['Cout'],), dtype=torch.float32, device='cuda')
            gemm_ms(A, B, bias, 2)
            d = sorted(gemm_ms(A, B, bias, 12) - gemm_ms(A, B, bias, 2) for _ in range(3))
            row['gemm_us'] = 1e3 * d[1] / 10
            del A, B
        res['layers'].append(row)
    eng.debug_set('debug_gemm_b3', None)
    # conv1_1 has no replay entry (it reads the caller's images): the forward minus the replayed layers
    rest = sum(r['us'] for r in res['layers'] if r['us'] is not None)
    res['layers'][0]['us'] = max(res['median_ms'] * 1e3 - rest, 0.0)
    res['layers'][0]['by_difference'] = True
    print('RESULT ' + json.dumps(res), flush=True)


def run_child(N, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(N), '--reps', str(reps)],
                         capture_output=True, text=True, timeout=420)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
        raise SystemExit('measurement N=%d failed with status %d: stopping' % (N, out.returncode))
    line = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', type=int, default=0)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vgg_pool5.md'))
    ap.add_argument('--run-label', default='one run of this tool on one MI355X')
    a = ap.parse_args()
    if a.child:
        return child(a.child, max(5, a.reps))
    results = [run_child(N, a.reps) for N in NS]
    with open(a.out, 'w') as f:
        f.write('# VGG-16 pool5 feature extraction: measured cost\n\n')
        f.write('`python tools/vgg_pool5_time.py`, %s: every figure below comes from that one run.  320 x 480 uint8 '
                'images, seed-0 synthetic weights (the published checkpoint is not available; timings do not depend on '
                'the values), exact fp32.  Forward: HIP events around `VGGPool5.forward`, 3 warm-up + %d timed calls, '
                'median (10 %% .. 90 %%).  Layers: mean of 20 back-to-back launches inside one event pair '
                '(`n2nmn_vgg_debug_replay`); conv1_1 (it reads the caller\'s images, no replay entry) is the forward minus '
                'the sum of the others, so it also carries the launch gaps.  TFLOP/s = 2 M Cout 9 Cin over that time; '
                'peak = %.1f TFLOP/s fp32 MFMA.  Yardstick: `n2nmn_debug_gemm` at the same M, N = Cout, K = 9 Cin '
                '(12-launch call minus 2-launch call, over 10; median of 3).\n\n' % (a.run_label, max(5, a.reps), PEAK_TFLOPS))
        for r in results:
            f.write('## N = %d: %.3f ms per call (%.3f .. %.3f), %.3f ms per image, %.1f TFLOP/s end to end\n\n' % (
                r['N'], r['median_ms'], r['p10_ms'], r['p90_ms'], r['median_ms'] / r['N'],
                sum(l['flop'] for l in r['layers']) / (r['median_ms'] * 1e-3) / 1e12))
            f.write('| layer | M | Cin | Cout | us | TFLOP/s | of peak | GB/s | dense GEMM us | GEMM TFLOP/s | conv / GEMM rate |\n')
            f.write('|---|---|---|---|---|---|---|---|---|---|---|\n')
            for l in r['layers']:
                tf_ = l['flop'] / (l['us'] * 1e-6) / 1e12 if l['us'] else 0.0
                gb = l['bytes'] / (l['us'] * 1e-6) / 1e9 if l['us'] else 0.0
                g = l.get('gemm_us')
                f.write('| %s%s | %d | %d | %d | %.1f | %s | %s | %.0f | %s | %s | %s |\n' % (
                    l['name'], ' (by difference)' if l.get('by_difference') else '', l['M'], l['Cin'], l['Cout'], l['us'],
                    '%.1f' % tf_ if l['flop'] else '-', '%.2f' % (tf_ / PEAK_TFLOPS) if l['flop'] else '-', gb,
                    '%.1f' % g if g else '-', '%.1f' % (l['flop'] / (g * 1e-6) / 1e12) if g else '-',
                    '%.2f' % (g / l['us']) if g else '-'))
            f.write('\n')
    print('wrote', a.out)
    print(open(a.out).read())


if __name__ == '__main__':
    main()
