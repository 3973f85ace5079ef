"""Cost of ResNet-152 res5c feature extraction (include/n2nmn.h section 10) at 448 x 448, N = 1, 8 and 32 images:
ms per image of ResNetRes5c.forward (HIP events around each call: 3 warm-up calls, `--reps` timed, median and the
10 % .. 90 % spread), of the whole network re-launched back to back (n2nmn_resnet_debug_replay with no layer
name), and per layer the mean time of one launch (the same entry with a name: 3 warm-up + 20 launches inside one
event pair).  Layers are summed per class -- stem, pool, 1x1, 3x3 -- and per stage; TFLOP/s is the algorithm's
2 M Cout k k Cin operations over that time, set against the 157.3 TFLOP/s fp32 MFMA peak.  Every measurement runs
in a child process of its own under a time limit; the first failure ends the run.  Writes profiles/resnet_replay.md.

    python tools/resnet_res5c_time.py [--reps 10] [--out profiles/resnet_replay.md] [--run-label TEXT]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
H, W = 448, 448
PEAK_TFLOPS = 157.3
NS = (1, 8, 32)


def layer_table(N):
    """name, cls, stage, M (output pixels), k, Cin, Cout, flop, bytes (activations read + written, weights)"""
    from n2nmn_amd import resnet
    half = lambda n: (n - 1) // 2 + 1
    ext = {1: (half(H), half(W))}
    ext[2] = (resnet.pool_extent(ext[1][0]), resnet.pool_extent(ext[1][1]))
    for s in (3, 4, 5):
        ext[s] = (half(ext[s - 1][0]), half(ext[s - 1][1]))
    rows = []
    for name, (k, _, cin, cout) in [(n[:-len('/weights')], s) for n, s in resnet.variable_shapes() if n.endswith('/weights')]:
        stage = 1 if name == 'conv1' else int(name[3])
        M = N * ext[stage][0] * ext[stage][1]
        cls = 'stem' if k == 7 else '3x3' if k == 3 else '1x1'
        res = M * cout if name.endswith('_branch2c') else 0
        rows.append(dict(name=name, cls=cls, stage=stage, M=M, k=k, Cin=cin, Cout=cout, flop=2.0 * M * cout * k * k * cin,
                         bytes=4.0 * (M * cin + M * cout + res + k * k * cin * cout)))
        if name == 'conv1':
            rows[0]['bytes'] = N * H * W * 3 + 4.0 * (M * cout + 147 * cout)            # uint8 input
            M2 = N * ext[2][0] * ext[2][1]
            rows.append(dict(name='pool1', cls='pool', stage=1, M=M2, k=3, Cin=cout, Cout=cout, flop=0.0,
                             bytes=4.0 * (M * cout + M2 * cout)))
    return rows


def child(N, reps):
    import numpy as np
    import torch
    from n2nmn_amd import resnet
    net = resnet.ResNetRes5c(max_N=N, max_H=H, max_W=W)
    net.load_weights(resnet.synthetic_weights(0))
    im = torch.as_tensor(np.random.RandomState(1).randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)).cuda()
    for _ in range(3):
        out = net.forward(im)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, 14, 14, 2048) and bool(torch.isfinite(out).all())
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); net.forward(im); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.sort(np.array(ms))
    res = dict(N=N, reps=reps, median_ms=float(np.median(ms)), p10_ms=float(ms[len(ms) // 10]),
               p90_ms=float(ms[-1 - len(ms) // 10]), replay_ms=net.replay_us('', 10) / 1e3, layers=[])
    for L in layer_table(N):
        res['layers'].append(dict(L, us=net.replay_us(L['name'], 20)))
    print('RESULT ' + json.dumps(res), flush=True)


def run_child(N, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(N), '--reps', str(reps)],
                         capture_output=True, text=True, timeout=420)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
        raise SystemExit('measurement N=%d failed with status %d: stopping' % (N, out.returncode))
    line = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def summed(layers, key):
    groups = {}
    for l in layers:
        g = groups.setdefault(key(l), dict(n=0, us=0.0, flop=0.0, bytes=0.0, M=l['M'], Cin=l['Cin'], Cout=l['Cout']))
        g['n'] += 1; g['us'] += l['us']; g['flop'] += l['flop']; g['bytes'] += l['bytes']
    return groups


def write_group_table(f, head, groups, total_us):
    f.write('| %s | launches | us | share | GFLOP | TFLOP/s | of peak | GB/s |\n|---|---|---|---|---|---|---|---|\n' % head)
    for k, g in groups.items():
        tf_ = g['flop'] / (g['us'] * 1e-6) / 1e12
        f.write('| %s | %d | %.1f | %.1f %% | %.2f | %s | %s | %.0f |\n' % (
            k, g['n'], g['us'], 100.0 * g['us'] / total_us, g['flop'] / 1e9, '%.1f' % tf_ if g['flop'] else '-',
            '%.2f' % (tf_ / PEAK_TFLOPS) if g['flop'] else '-', g['bytes'] / (g['us'] * 1e-6) / 1e9))
    f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', type=int, default=0)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resnet_replay.md'))
    ap.add_argument('--run-label', default='one run of this tool on one MI355X')
    a = ap.parse_args()
    if a.child:
        return child(a.child, max(5, a.reps))
    results = [run_child(N, a.reps) for N in NS]
    with open(a.out, 'w') as f:
        f.write('# ResNet-152 res5c feature extraction: measured cost\n\n')
        f.write('`python tools/resnet_res5c_time.py`, %s: every figure in the tables below comes from that one run.  '
                '448 x 448 uint8 images, seed-0 synthetic weights (the published ones are not available; timings do not '
                'depend on the values), exact fp32.  Forward: HIP events around `ResNetRes5c.forward`, 3 warm-up + %d '
                'timed calls, median (10 %% .. 90 %%).  Replay: the whole network 10 times back to back inside one event '
                'pair (`n2nmn_resnet_debug_replay`, no layer name).  Layers: mean of 20 back-to-back launches of one '
                'layer inside one event pair (the same entry, with a name), summed per class and per stage; the first '
                'branch2a of a stage carries the clearing of its output buffer.  TFLOP/s = 2 M Cout k k Cin over that '
                'time; peak = %.1f TFLOP/s fp32 MFMA.  GB/s = activations read and written plus weights, once each, over '
                'that time (back-to-back launches re-read from L2 / MALL: not an HBM figure).\n\n'
                % (a.run_label, max(5, a.reps), PEAK_TFLOPS))
        for r in results:
            flop = sum(l['flop'] for l in r['layers'])
            total_us = sum(l['us'] for l in r['layers'])
            f.write('## N = %d: forward %.3f ms per call (%.3f .. %.3f), %.3f ms per image, %.1f TFLOP/s end to end\n\n' % (
                r['N'], r['median_ms'], r['p10_ms'], r['p90_ms'], r['median_ms'] / r['N'], flop / (r['median_ms'] * 1e-3) / 1e12))
            f.write('Whole-network replay: %.3f ms per round, %.3f ms per image.  Sum of the %d single-layer replays: %.3f ms '
                    '(%.2f GFLOP per image).\n\n' % (r['replay_ms'], r['replay_ms'] / r['N'], len(r['layers']), total_us / 1e3,
                                                   flop / r['N'] / 1e9))
            write_group_table(f, 'class', summed(r['layers'], lambda l: l['cls']), total_us)
            write_group_table(f, 'stage / class (M x Cin -> Cout of its first layer)',
                              {'%s (%d x %d -> %d)' % (k, g['M'], g['Cin'], g['Cout']): g for k, g in
                               summed(r['layers'], lambda l: ('conv1 / pool1' if l['stage'] == 1 else 'res%d' % l['stage'])
                                      + ' ' + l['cls']).items()}, total_us)
            f.write('Slowest single layers:\n\n| layer | M | Cin | Cout | us | TFLOP/s | of peak |\n|---|---|---|---|---|---|---|\n')
            for l in sorted(r['layers'], key=lambda l: -l['us'])[:8]:
                tf_ = l['flop'] / (l['us'] * 1e-6) / 1e12
                f.write('| %s | %d | %d | %d | %.1f | %.1f | %.2f |\n' % (l['name'], l['M'], l['Cin'], l['Cout'], l['us'], tf_,
                                                                     tf_ / PEAK_TFLOPS))
            f.write('\n')
    print('wrote', a.out)
    print(open(a.out).read())


if __name__ == '__main__':
    main()
