#!/usr/bin/env python3
"""Benchmark of the N2NMN CLEVR forward hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: the script re-executes itself under torch.distributed.run, one rank per GPU; when the
     driver already launched it that way, RANK / LOCAL_RANK / WORLD_SIZE come from the environment)

A plain run does only what the headline figure needs: set-up, the warm-up passes, the `--steps` timed
passes, the `--dump-outputs` arrays and the result line.  `--full` adds, after the timed region, everything
else this script measures or checks: `parity_check`, `single_batch`, `config3`, `eos_retire`, `bf16x3`,
the per-kernel `roofline` / `roofline_attention` / `kernels` tables, `config4` / `config5` and
`cpu_baseline` (for `--config 4 | 5 | 6`: their kernel tables, CPU baseline and extra passes).
`--no-profile` / `--no-cpu-baseline` leave parts of it out again.

One "step" = ONE PASS of the hot path (BASELINE.json configs[1]: CLEVR forward, fixed ground-truth
layouts, 10x15x512 synthetic pool5 features) over `--inflight K` client batches of 64 questions that
share every launch of the pass (super-bucketing, n2nmn_amd/superbucket.py):
phase 1 (LSTM encoder + teacher-forced attentional decoder), hoisted conv_image GEMMs, and the layout
walker, which decodes the layouts on the device and runs every question's module tree -> answer
logits in HBM.  Nothing synchronises inside a step (no token fetch, no host assembly, no upload).

Throughput number (`value`): `--streams S` workers (pre-spawned host thread + HIP stream + forked
context each, shared weights; n2nmn_amd/pipeline.py -- the object tests/test_gpu_bench_config.py
checks against the oracle) run passes concurrently, each alternating two buckets of distinct inputs;
exactly `--steps` passes are timed, split evenly over the workers; value = K * 64 * steps / time.
`config` says what a launch carried (`rows_per_launch`, `questions_in_flight`).  Default: 2 streams,
K = 16 (1024 rows per launch; round 5's sweep: 2 / 3 / 4 streams = 311 / 316 / 301 k questions/s -- 3 is not
the default because the 3-worker form of tests/test_gpu_bench_config.py failed in 2 of 5 runs in the bf16x3
mode -- a 3e-4 logit error on one worker's pass, not reproduced in isolation: profiles/r05_notes.md section 8).
With `--full`: `parity_check`: logits of the timed passes against the oracle.
Latency number (`single_batch`): one batch of 64 in flight (the strict reading of "batch 64").
`config3`: the same with layouts chosen by the greedy decoder (BASELINE.json configs[2]).
`config4` / `config5`: the training step and the models_vqa forward (BASELINE.json configs[3], [4]),
one GPU, so the `--full` line carries them too (`--config 4|5|6` runs them alone).

Inputs are resident in HBM before the timed region.  Multi-GPU: the path shards by question with no
data-path collective (weak scaling: every rank runs its own stream of batches); timing =
barrier + synchronize on both sides, max over ranks (`timed_region_s`).

`--dump-outputs DIR`: after the timed passes, what the last timed pass of every worker handed its caller
(answer logits, layout tokens, layout validity) is written as DIR/<name>.npy (float32; rank 0).  The
inputs are seeded, so two builds run with the same arguments can be compared output for output.

Prints ONE JSON line on rank 0: the headline figures and a summary of every sub-report (result_line);
the full report, per-kernel tables included, goes to stderr as one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
L2_PEAK_GBS = 34500.0       # MI355X_MICROARCH.md: aggregate L2 bandwidth (8 XCDs)
# dec_attn re-reads the encoder rows of a question from L2/MALL (PMC: 17 MB of HBM traffic for 236 MB of
# algorithmic bytes per launch); the answer heads / fc_att groups and the text-map kernels stream weight
# matrices and tables that live in L2
L2_FAMILIES = ('dec_attn', 'heads', 'walk_tmap', 'textmap')
MFMA_F32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: fp32-input MFMA dense peak
MFMA_FAMILIES = ('lstm_step', 'gemm_pk', 'lstm_bwd_step', 'gemm_tn')


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--config', type=int, default=2, choices=(2, 3, 4, 5, 6),
                    help='2: fixed gt layouts (metric config); 3: greedy decoder layouts; '
                         '4: training step (forward + backward + RCCL all-reduce + Adam); '
                         '5: models_vqa forward (14x14x2048 feats, batch 128); '
                         '6: models_vqa training step (batch 64, dropout, Adam)')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--inflight', type=int, default=16,
                    help='batches of --batch questions super-bucketed into one pass (1..16)')
    ap.add_argument('--streams', type=int, default=2,
                    help='independent super-buckets in flight per GPU (one pre-spawned host thread + '
                         'HIP stream + forked context each; weights shared)')
    ap.add_argument('--host-assemble', action='store_true',
                    help='reference flow: token fetch + C++ Assembler + level scheduler instead of '
                         'the on-device layout walker')
    extent = ap.add_mutually_exclusive_group()
    extent.add_argument('--full', action='store_true',
                        help='after the timed region, also run every other measurement and check of this '
                             'script (oracle parity, single batch, config3, eos_retire, bf16x3, per-kernel '
                             'tables, config4 / config5, cpu baseline); off: the headline figure alone')
    extent.add_argument('--plain', action='store_true',
                        help='only the timed throughput region: what a run without --full does (kept for the '
                             'commands the rocprofv3 traces in profiles/ were taken with)')
    ap.add_argument('--lstm-mode', default=None, choices=(None, 'throughput', 'throughput_bf16x3'),
                    help="recurrent-step mode of the timed passes; 'throughput_bf16x3' = the opt-in "
                         "split-operand bf16 mode (NOT the headline: `dtype` then reads 'bf16x3 (fp32-"
                         "equivalent)'; the --full line reports it under the `bf16x3` key)")
    ap.add_argument('--eos-retire', action='store_true',
                    help='timed passes with the inference option N2NMN_S2S_EOS_RETIRE (NOT the headline: the '
                         'metric text and config.eos_retire say so; the --full line reports it under the '
                         '`eos_retire` key).  For rocprofv3 traces of the retired pass')
    ap.add_argument('--layouts', default='templates', choices=('templates', 'clevr_like'),
                    help="ground-truth layout mix of the timed passes ('clevr_like': synth.clevr_like_layout_batch)")
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: no cpu_baseline')
    ap.add_argument('--no-profile', action='store_true', help='with --full: no per-kernel tables')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed passes, write what the last timed pass of every worker computed '
                         '(scores, tokens, validity; rank 0) as DIR/<name>.npy (--config 2 / 3)')
    return ap.parse_args(argv)


PMC_FILE = os.path.join(ROOT, 'profiles', 'r06_pmc_traffic.json')
for _older in ('r05_pmc_traffic.json', 'r04_pmc_traffic.json'):
    if not os.path.exists(PMC_FILE):
        PMC_FILE = os.path.join(ROOT, 'profiles', _older)
# hardware MFMA counters of the same bench commands (tools/pmc_mfma.sh: SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE and
# SQ_INSTS_VALU_MFMA_MOPS_*): per kernel the matrix-pipe busy fraction and the flops the counters saw
PMC_MFMA_FILE = {'fwd': os.path.join(ROOT, 'profiles', 'r06_pmc_mfma_fwd.json'),
                 'trn': os.path.join(ROOT, 'profiles', 'r06_pmc_mfma_trn.json')}
PMC_FILE_TRAIN = os.path.join(ROOT, 'profiles', 'r01_pmc_traffic_train.json')
PMC_KERNEL = {'lstm_step': 'lstm_tile_kernel', 'dec_attn': 'dec_attn_question_kernel',
              'pool': 'walk_pool_kernel', 'walk_find': 'walk_find', 'walk_tmap': 'walk_tmap_kernel',
              'gemm_pkn': 'gemm_dma_kernel', 'gemm_pk': 'gemm_pk', 'att_ops': 'att_ops_kernel',
              'textmap': 'walk_textmap_kernel', 'heads': 'heads_kernel', 'word_vecs': 'word_vecs_kernel',
              # the staged walker: Transform / FindSameProperty jobs + the per-question rest + the fall-back launch
              'walk(': ('walk_heavy_kernel', 'walk_fspepi_kernel', 'walk_light_kernel', 'walk_kernel'),
              'lstm_bwd_step': 'lstm_bwd_step_kernel', 'gemm_tn': 'gemm_tn_kernel',
              'optimiser': 'adam_kernel'}


def pmc_traffic(family, path=None):
    """HBM bytes per launch of the kernel behind a profiler family, from the committed rocprofv3
    PMC passes (tools/pmc_traffic.py: separate FETCH_SIZE / WRITE_SIZE runs of this same bench
    command, gfx950 x2 read correction).  PMC counters cannot be read inside the timed run."""
    try:
        data = json.load(open(path or PMC_FILE))['kernels']
        for prefix, kname in PMC_KERNEL.items():
            names = kname if isinstance(kname, tuple) else (kname,)
            hit = [k for n in names for k in data if k.startswith(n)][:len(names)]   # (template arguments vary)
            if family.startswith(prefix) and hit:
                return sum(data[k]['hbm_bytes_per_launch'] for k in hit), \
                    'profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)' % \
                    os.path.basename(path or PMC_FILE)
    except Exception:
        pass
    return None, None


def pmc_mfma(family, which='fwd', encoder_launches=None):
    """{'mfma_busy', 'counter_flops_per_launch', 'from_file'} of the kernel behind a profiler family, from the committed
    rocprofv3 --pmc passes (counters cannot be read inside the timed run); {} when the file or the kernel is missing."""
    try:
        data = json.load(open(PMC_MFMA_FILE[which]))
        # (both big GEMMs of a pass -- conv_image and the phase-1 GEMM -- run on gemm_dma_kernel at these shapes;
        # gemm_pk_kernel only serves the handful of set-up products)
        for prefix, kname in dict(PMC_KERNEL, gemm_pk='gemm_dma_kernel').items():
            names = kname if isinstance(kname, tuple) else (kname,)
            hit = [k for n in names for k in data if k.startswith(n)][:1]
            if family.startswith(prefix) and hit:
                r = data[hit[0]]
                out = {'mfma_busy': round(r['mfma_busy'], 4), 'kernel': hit[0], 'launches_counted': r['launches'],
                       'from_file': 'profiles/%s (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE; '
                                    'SQ_INSTS_VALU_MFMA_MOPS_F32 x 512, separate passes)' %
                                    os.path.basename(PMC_MFMA_FILE[which])}
                fl = r.get('counter_flops_f32', 0.0) + r.get('counter_flops_bf16', 0.0)
                if fl:
                    out['counter_flops_per_launch'] = round(fl)
                return out
    except Exception:
        pass
    return {}


def cpu_baseline(d, w, names, use_gt, gpu_scores_fn):
    """batched torch-CPU port mirroring TF's op granularity and Fold's per-(module,
    depth) batching (oracle/n2nmn_oracle_batched.py; the reference's TF1 path cannot run here), fp32,
    all host threads; 3 warm-up batches, then batches until ~20 are timed (capped at 30 s), median
    q/s, same seeded inputs as the GPU run, logits asserted equal to the GPU's in this process."""
    import numpy as np
    import torch
    from n2nmn_amd import synth
    from oracle import n2nmn_oracle_batched as OB
    wt = OB.to_torch(w, torch.float32)
    # thread count: the ops of one batch are small (a [64, 812] x [812, 2048] matmul per cell and
    # step); on a 256-thread host all-threads runs ~250x slower than 16 threads, so one batch is
    # tried at a few settings and the fastest is timed (what a tuned intra-op pool would give)
    b0 = synth.make_inputs(d, seed=999)
    gt0 = synth.template_layout_batch(d) if use_gt else None
    ncpu = os.cpu_count() or 1
    best, trial = None, {}
    for nt in sorted({min(ncpu, t) for t in (8, 16, 32, 64)}):
        torch.set_num_threads(nt)
        t0 = time.perf_counter()
        OB.forward(wt, names, b0, d.T_decoder, d.num_choices, use_gt, gt0)
        trial[nt] = time.perf_counter() - t0
        if best is None or trial[nt] < trial[best]:
            best = nt
        if trial[nt] > 8.0:
            break
    torch.set_num_threads(best)
    times, worst = [], 0.0
    t_all = time.perf_counter()
    i = 0
    while len(times) < 20 and time.perf_counter() - t_all < 25.0:
        b = synth.make_inputs(d, seed=1000 + i)
        gt = synth.template_layout_batch(d, offset=i) if use_gt else None
        t0 = time.perf_counter()
        out = OB.forward(wt, names, b, d.T_decoder, d.num_choices, use_gt, gt)
        dt = time.perf_counter() - t0
        if i >= 3 or dt > 3.0:
            times.append(dt)
        if i < 2:                                      # parity of the timed port against the GPU
            got = gpu_scores_fn(b, gt)
            worst = max(worst, float(np.abs(got - out['scores']).max()))
            assert worst < 1e-3, 'cpu_baseline port and GPU disagree: %.3e' % worst
        i += 1
    med = sorted(times)[len(times) // 2]
    try:
        model = [l.split(':', 1)[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name')][0]
    except Exception:
        model = 'unknown'
    return {'value': round(d.N / med, 2), 'unit': 'questions/sec', 'cores': int(torch.get_num_threads()),
            'kind': 'port',
            'sample': '%d batches of %d questions after warm-ups, median; batched torch-CPU fp32 port '
                      '(oracle/n2nmn_oracle_batched.py: one matmul per LSTM cell and step, conv2d for '
                      'Transform, one call per (module, depth) like TF-Fold), %d threads (fastest of %s s '
                      'per batch) on %d host cores (%s); max |logit diff| vs the GPU on the same '
                      'inputs %.1e; the reference TF1/Fold CPU path is not runnable here' %
                      (len(times), d.N, torch.get_num_threads(),
                       {k: round(v, 2) for k, v in trial.items()}, ncpu, model, worst)}


def kernel_rows(fams, ksteps, overhead_us=0.0):
    """per kernel family: HIP-event time per launch (an event pair reads ~1.5-2 us more than
    rocprofv3's kernel duration for these kernels: profiles/); fractions are therefore conservative."""
    rows = []
    for f in fams:
        if f['launches'] == 0:
            continue
        bound = 'mfma' if f['name'].startswith(MFMA_FAMILIES) else \
            ('l2' if f['name'].startswith(L2_FAMILIES) else 'hbm')
        raw_s = f['total_ms'] * 1e-3 / f['launches']
        avg_s = raw_s
        if bound == 'mfma':
            ach = f['flops'] / f['launches'] / avg_s / 1e12
            peak, unit = MFMA_F32_PEAK_TF, 'TFLOP/s'
        else:
            ach = f['bytes'] / f['launches'] / avg_s / 1e9
            peak, unit = (L2_PEAK_GBS if bound == 'l2' else HBM_PEAK_GBS), 'GB/s'
        rows.append({'kernel': f['name'], 'bound': bound, 'launches_per_step':
                     round(f['launches'] / ksteps, 2), 'avg_us': round(avg_s * 1e6, 3),
                     'us_per_step': round(avg_s * 1e6 * f['launches'] / ksteps, 2),
                     'achieved': round(ach, 3), 'peak': peak, 'unit': unit,
                     'frac': round(ach / peak, 4)})
    rows.sort(key=lambda r: -r['us_per_step'])
    return rows


def bench_train(args, dp, local_rank):
    out = train_numbers(args, dp, local_rank, args.steps, args.warmup, not args.no_profile,
                        not args.no_cpu_baseline)
    if dp.rank == 0:
        emit_report(out)
    dp.close()


def train_numbers(args, dp, local_rank, steps, warmup, profile=True, cpu=True):
    """BASELINE.json configs[3]: exp_clevr/train_clevr_gt_layout.py loop body -- forward + backward
    + gradient all-reduce (RCCL, two buckets, the late one overlapping the encoder's backward) +
    per-tensor clip + Adam -- batch 64 per GPU, T_dec = 10, gt layouts.  One step = one iteration."""
    import numpy as np
    import torch
    from n2nmn_amd import synth
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
    from n2nmn_amd.train import Trainer

    rank, world = dp.rank, dp.world
    d = Dims(N=args.batch, T_decoder=10)
    names = list(CLEVR_MODULE_NAMES)
    eng = Engine(d, Assembler(names), device=local_rank)
    w = synth.make_weights(d, seed=0)          # identical replicas on every rank
    eng.load_weights(w)
    dev = eng.device
    # one rank: no process group on the data path at all (a 1-rank RCCL communicator would only add
    # its start-up banner to this script's one-line stdout)
    tr = Trainer(eng, dist=dp._dist if world > 1 else None)
    n_batches = 4
    batches, gts = [], []
    for i in range(n_batches):
        b = synth.make_inputs(d, seed=dp.batch_seed(i))
        batches.append({k: torch.as_tensor(v).to(dev) for k, v in b.items()})
        gts.append(synth.template_layout_batch(d, offset=i))      # host: assembled per step

    def run_steps(first, count):
        for i in range(first, first + count):
            tr.step(batches[i % n_batches], gts[i % n_batches])

    run_steps(0, warmup)
    elapsed = dp.timed(lambda: run_steps(warmup, steps),
                       sync=lambda: torch.cuda.synchronize(dev))
    out = None
    if rank == 0:
        out = {
            'metric': 'questions/sec (training step: forward + backward + all-reduce + Adam) on '
                      'CLEVR 10x15x512 feats, batch 64 per GPU',
            'value': round(dp.throughput(d.N * steps, elapsed), 1), 'unit': 'questions/sec',
            'n_gpus': world, 'steps': steps, 'warmup': warmup,
            'ms_per_step': round(1e3 * elapsed / steps, 4), 'higher_is_better': True,
            'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': 'BASELINE.json configs[3]: CLEVR train_clevr_gt_layout.py step, '
                                   'gt layouts (10-template mix), batch %d per GPU, T_enc=45, '
                                   'T_dec=10, weight_decay 5e-6, clip 10, Adam' % d.N,
                       'global_batch': world * d.N,
                       'parallelism': 'dp%d: flat fp32 gradient (%d floats), 2 RCCL all-reduce '
                                      'buckets per step' % (world, tr.numel)},
            'final_total_loss': float(tr.losses[3].item()),
            # which all-reduce ran, and over how many ranks BY THE COMMUNICATOR'S OWN ACCOUNT (an
            # all-reduce of ones at construction + n2nmn_comm_world), not WORLD_SIZE
            'bucket_impl': tr.bucket_impl, 'rccl_ranks': tr.rccl_ranks,
        }
    if rank == 0 and profile and world == 1:
        ksteps = min(steps, 20)
        eng.profile_begin()
        run_steps(0, ksteps)
        rows = kernel_rows(eng.profile_end(), ksteps)
        dom = rows[0]
        out['roofline'] = {'kernel': dom['kernel'], 'bound': dom['bound'],
                           'achieved': dom['achieved'], 'peak': dom['peak'], 'unit': dom['unit'],
                           'frac': dom['frac'], 'traffic': pmc_traffic(dom['kernel'], PMC_FILE_TRAIN)[0],
                           'traffic_source': pmc_traffic(dom['kernel'], PMC_FILE_TRAIN)[1],
                           'avg_us': dom['avg_us'],
                           'measured': 'hipEvent pairs around each launch, separate pass of %d '
                                       'steps' % ksteps}
        # hardware MFMA counters of the step's matrix kernels next to the library's own flop counts
        for r in rows:
            if r['bound'] == 'mfma':
                hw = pmc_mfma(r['kernel'], 'trn')
                if hw:
                    own = r['achieved'] * 1e12 * r['avg_us'] * 1e-6
                    if r['kernel'].startswith('gemm_pk'):
                        # rocprofv3 groups by kernel name: the counter mean is over BOTH gemm_dma launches of a pass
                        grp = [x for x in rows if x['kernel'].startswith('gemm_pk') and x['bound'] == 'mfma']
                        n_l = sum(x['launches_per_step'] for x in grp)
                        own = sum(x['achieved'] * 1e12 * x['avg_us'] * 1e-6 * x['launches_per_step'] for x in grp) / max(n_l, 1)
                        hw['library_flops_per_launch_same_launch_set'] = round(own)
                    if hw.get('counter_flops_per_launch'):
                        hw['counter_over_library'] = round(hw['counter_flops_per_launch'] / max(own, 1.0), 4)
                    r['mfma_counters'] = hw
        out['kernels'] = rows
        out['gpu_us_per_step'] = round(sum(r['us_per_step'] for r in rows), 1)
    if rank == 0 and world == 1 and cpu:
        from oracle import n2nmn_oracle_grad as G
        b0 = synth.make_inputs(d, seed=0)
        t0 = time.perf_counter()
        G.loss_and_grads(w, names, b0, d.T_decoder, d.num_choices,
                         synth.template_layout_batch(d), 5e-6)
        dt = time.perf_counter() - t0
        out['cpu_baseline'] = {'value': round(d.N / dt, 2), 'unit': 'questions/sec',
                               'cores': int(torch.get_num_threads()), 'kind': 'port',
                               'sample': '1 batch of %d questions, forward+backward of the torch-'
                                         'autograd fp64 oracle (oracle/n2nmn_oracle_grad.py), no '
                                         'optimiser step; the reference TF1/Fold path is not '
                                         'runnable here' % d.N}
    return out


def bench_vqa(args, dp, local_rank):
    out = vqa_numbers(args, dp, local_rank, args.steps, args.warmup, not args.no_profile, per_pass_coords=args.full)
    if args.full and args.batch == 64:
        p = vqa_numbers(args, dp, local_rank, max(3, args.steps // 8), 2, False, batches_per_pass=8)
        if dp.rank == 0:
            out['passes'] = {k: p[k] for k in ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'config')}
        pd = vqa_numbers(args, dp, local_rank, max(3, args.steps // 8), 2, not args.no_profile, batches_per_pass=8,
                         device_layouts=True)
        if dp.rank == 0:
            out['passes_device_layouts'] = {k: pd[k] for k in ('value', 'ms_per_step', 'steps', 'host_sync', 'kernels')
                                            if k in pd}
    if dp.rank == 0:
        emit_report(out)
    dp.close()


def vqa_numbers(args, dp, local_rank, steps, warmup, profile=True, batches_per_pass=1, lstm_mode=None,
                device_layouts=False, eos_retire=False, per_pass_coords=True):
    """BASELINE.json configs[4]: models_vqa forward (exp_vqa/eval_vqa2.py:103-137) -- seq2seq with
    the 17742-word vocabulary and lstm_dim 1000, coordinate map, the 4-module network at map_dim
    1024 on 14x14x2048 features, question prior net -- batch 128 per GPU, ground-truth layouts from
    the v2 validation histogram.  batches_per_pass > 1: that many client batches of 128
    as one pass (every launch carries batches_per_pass * 128 rows; recurrent step in 'throughput'
    mode), the serving form of the headline configuration.  per_pass_coords: time the single-batch passes a
    second time with the coordinate channels appended per pass (`with_per_pass_add_coords`)."""
    import numpy as np
    import torch
    from n2nmn_amd import synth, vqa
    rank, world = dp.rank, dp.world
    client = 128 if args.batch == 64 else args.batch
    d = vqa.VQADims(N=client * batches_per_pass)
    eng = vqa.VQAEngine(d, device=local_rank)
    w = synth.make_weights_from_shapes(vqa.vqa_variable_shapes(d), seed=0)
    eng.load_weights(w)
    mode = lstm_mode or ('throughput' if batches_per_pass > 1 else None)
    if mode:
        eng.engine.set_mode(mode)
    dev = eng.engine.device
    mix = (['_Find', '_Find', '_And', '_Describe'],) * 46 + (['_Find', '_Describe'],) * 43 + \
          (['_Find', '_Transform', '_Describe'],) * 9 + (['_Find', '_Transform', '_Find', '_And', '_Describe'],) * 2
    rng = np.random.default_rng(dp.batch_seed(0))
    batches, gts = [], []
    for i in range(3):
        lens = rng.integers(3, d.T_encoder + 1, size=d.N).astype(np.int32)
        seq = rng.integers(0, d.num_vocab_txt, size=(d.T_encoder, d.N)).astype(np.int32)
        seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
        feat = torch.relu(torch.randn((d.N, d.H, d.W, d.D), generator=torch.Generator().manual_seed(i)))
        # inputs resident in HBM in the engine's input layout: a slab [N, 14, 14, 2064] whose two coordinate
        # channels (constants of add_spatial_coordinate_map) were written once; the client's copy fills the
        # 2048 image channels -- outside the timed region, like every input of this bench
        slab = eng.feature_slab(d.N)
        slab[..., :d.D].copy_(feat.to(dev))
        batches.append(dict(input_seq_batch=torch.as_tensor(seq).to(dev),
                            seq_length_batch=torch.as_tensor(lens).to(dev),
                            image_feat_batch=slab))
        order = rng.permutation(100)
        # host arrays, as the reference's data reader delivers gt_layout_batch: the program is
        # assembled from them up front and nothing synchronises inside a step
        gts.append(np.ascontiguousarray(np.array(
            [eng.assembler.module_list2tokens(mix[order[n % 100]], d.T_decoder) for n in range(d.N)],
            np.int32).T))

    gts_dev = [torch.as_tensor(g).to(dev) for g in gts]

    def run_steps(first, count):
        for i in range(first, first + count):
            if device_layouts:
                eng.forward(batches[i % 3], use_gt_layout=True, gt_layout=gts_dev[i % 3], fetch=False,
                            eos_retire=eos_retire)
            else:
                eng.forward(batches[i % 3], use_gt_layout=True, gt_layout=gts[i % 3], eos_retire=eos_retire)

    run_steps(0, warmup)
    elapsed = dp.timed(lambda: run_steps(warmup, steps),
                       sync=lambda: torch.cuda.synchronize(dev))
    # the same passes with the features as plain [N, 14, 14, 2048] tensors: add_spatial_coordinate_map's work
    # (models_vqa/nmn3_modules.py:11-31, inside the reference's graph) is then done per pass by n2nmn_add_coords --
    # the figure comparable with rounds 1-4
    elapsed_coords = None
    if per_pass_coords and batches_per_pass == 1 and not device_layouts and not eos_retire:
        slabs = batches
        batches = [dict(b, image_feat_batch=b['image_feat_batch'][..., :d.D].contiguous()) for b in slabs]
        run_steps(0, warmup)
        elapsed_coords = dp.timed(lambda: run_steps(warmup, steps), sync=lambda: torch.cuda.synchronize(dev))
        batches = slabs
    out = None
    if rank == 0:
        label = 'batch %d per GPU' % d.N if batches_per_pass == 1 else \
            'client batches of %d served as passes of %d rows (throughput)' % (client, d.N)
        out = {'metric': 'questions/sec (forward) on VQAv2 14x14x2048 feats, ' + label,
               'value': round(dp.throughput(d.N * steps, elapsed), 1), 'unit': 'questions/sec',
               'n_gpus': world, 'steps': steps, 'warmup': warmup,
               'ms_per_step': round(1e3 * elapsed / steps, 4), 'higher_is_better': True,
               'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
               'config': {'workload': 'BASELINE.json configs[4]: models_vqa forward, gt layouts (v2 val '
                                      'histogram), %s, T_enc=26, T_dec=13, single stream, %s' % (
                                          label, 'layouts as device tokens: assembled + level-scheduled on the GPU'
                                          if device_layouts else 'layouts as host arrays: program assembled up front'),
                          'client_batch': client, 'batches_per_pass': batches_per_pass,
                          'rows_per_launch': d.N, 'lstm_step_mode': mode or 'latency',
                          'global_batch': world * d.N,
                          'input_layout': 'features resident in HBM as the engine\'s slab [N, 14, 14, 2064]: 2048 image '
                                          'channels + the 2 coordinate channels of add_spatial_coordinate_map (constants, '
                                          'written once per slab: VQAEngine.feature_slab) + zero padding; no per-pass '
                                          'n2nmn_add_coords',
                          'parallelism': 'dp%d (question-sharded)' % world},
               'host_sync': 'none: tokens never leave the GPU between the phases (n2nmn_execute_tokens)'
               if device_layouts else 'none: gt_layout_batch is a host array, the program is assembled before phase 1'}
        if elapsed_coords is not None:
            out['with_per_pass_add_coords'] = {
                'value': round(dp.throughput(d.N * steps, elapsed_coords), 1), 'unit': 'questions/sec',
                'ms_per_step': round(1e3 * elapsed_coords / steps, 4),
                'input_layout': 'features as [N, 14, 14, 2048] tensors; the coordinate channels are appended per pass '
                                '(n2nmn_add_coords), as the reference does inside its graph'}
        if profile:
            ksteps = min(steps, 10)
            eng.engine.profile_begin()
            run_steps(0, ksteps)
            rows = kernel_rows(eng.engine.profile_end(), ksteps)
            out['kernels'] = rows
            out['gpu_us_per_step'] = round(sum(r['us_per_step'] for r in rows), 1)
    return out


def bench_vqa_train(args, dp, local_rank):
    """models_vqa training step (exp_vqa/train_vqa_gt_layout.py:27-39,148-190): batch 64 per GPU,
    encoder / decoder / question-prior dropout, forward + backward + Adam (no clipping), ground-truth
    layouts from the v2 histogram, 17742-word vocabulary, 3001 answers."""
    import numpy as np
    import torch
    from n2nmn_amd import synth, vqa
    rank, world = dp.rank, dp.world
    d = vqa.VQADims(N=args.batch)
    eng = vqa.VQAEngine(d, device=local_rank)
    eng.load_weights(synth.make_weights_from_shapes(vqa.vqa_variable_shapes(d), seed=0))
    dev = eng.engine.device
    tr = vqa.VQATrainer(eng, dist=dp._dist)
    mix = (['_Find', '_Find', '_And', '_Describe'],) * 46 + (['_Find', '_Describe'],) * 43 + \
          (['_Find', '_Transform', '_Describe'],) * 9 + (['_Find', '_Transform', '_Find', '_And', '_Describe'],) * 2
    rng = np.random.default_rng(dp.batch_seed(0))
    batches, gts = [], []
    for i in range(3):
        lens = rng.integers(3, d.T_encoder + 1, size=d.N).astype(np.int32)
        seq = rng.integers(0, d.num_vocab_txt, size=(d.T_encoder, d.N)).astype(np.int32)
        seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
        feat = torch.relu(torch.randn((d.N, d.H, d.W, d.D), generator=torch.Generator().manual_seed(i)))
        batches.append(dict(input_seq_batch=torch.as_tensor(seq).to(dev),
                            seq_length_batch=torch.as_tensor(lens).to(dev),
                            image_feat_batch=feat.to(dev),
                            answer_label_batch=torch.as_tensor(
                                rng.integers(0, d.num_choices, size=d.N).astype(np.int32)).to(dev)))
        order = rng.permutation(100)
        gts.append(np.array([eng.assembler.module_list2tokens(mix[order[n % 100]], d.T_decoder)
                             for n in range(d.N)], np.int32).T.copy())

    def run_steps(first, count):
        for i in range(first, first + count):
            tr.step(batches[i % 3], gts[i % 3])

    run_steps(0, args.warmup)
    elapsed = dp.timed(lambda: run_steps(args.warmup, args.steps),
                       sync=lambda: torch.cuda.synchronize(dev))
    if rank == 0:
        out = {'metric': 'questions/sec (training step) on VQAv2 14x14x2048 feats, batch %d per GPU' % d.N,
               'value': round(dp.throughput(d.N * args.steps, elapsed), 1), 'unit': 'questions/sec',
               'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
               'ms_per_step': round(1e3 * elapsed / args.steps, 4), 'higher_is_better': True,
               'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
               'config': {'workload': 'models_vqa training step (exp_vqa/train_vqa_gt_layout.py): forward '
                                      '+ backward + Adam, dropout on, gt layouts (v2 histogram), batch %d '
                                      'per GPU, T_enc=26, T_dec=13' % d.N,
                          'global_batch': world * d.N, 'parallelism': 'dp%d' % world},
               'losses': [round(float(x), 4) for x in tr.losses[:4].cpu()]}
        if not args.no_profile:
            ksteps = min(args.steps, 5)
            eng.engine.profile_begin()
            run_steps(0, ksteps)
            rows = kernel_rows(eng.engine.profile_end(), ksteps)
            out['kernels'] = rows
            out['gpu_us_per_step'] = round(sum(r['us_per_step'] for r in rows), 1)
        emit_report(out)
    dp.close()


def spawn_command(args, argv):
    """The torch.distributed.run command that runs this script on args.gpus ranks of one node."""
    import socket
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        port = so.getsockname()[1]
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
            '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
            '--master-port', str(port), os.path.abspath(__file__)] + list(argv)


_RESULT_FD = None


def own_stdout():
    """The contract is ONE JSON line on stdout.  Libraries print there too (RCCL's version banner at
    communicator creation, under torch.distributed.run): from here on file descriptor 1 points at
    stderr and the result line goes to the saved descriptor."""
    global _RESULT_FD
    if _RESULT_FD is None:
        sys.stdout.flush()
        _RESULT_FD = os.dup(1)
        os.dup2(2, 1)


def emit_line(line):
    sys.stdout.flush()
    os.write(_RESULT_FD if _RESULT_FD is not None else 1, (line + '\n').encode())


def ensure_world(args, argv):
    """--gpus N must mean N ranks.  Under torch.distributed.run: WORLD_SIZE has to agree.  Otherwise
    N > 1 re-executes this script under torch.distributed.run, or fails if the node has < N GPUs."""
    ws = os.environ.get('WORLD_SIZE')
    if ws is not None:
        if int(ws) != args.gpus:
            sys.exit('bench.py: --gpus %d but launched with WORLD_SIZE=%s' % (args.gpus, ws))
        return
    if args.gpus <= 1:
        return
    import torch
    have = torch.cuda.device_count()
    if have < args.gpus:
        sys.exit('bench.py: --gpus %d needs %d devices, this node has %d' %
                 (args.gpus, args.gpus, have))
    cmd = spawn_command(args, argv)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    sys.stderr.write('bench.py: spawning %d ranks: %s\n' % (args.gpus, ' '.join(cmd)))
    os.execvp(cmd[0], cmd)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, pipe, steps):
    """--dump-outputs: what the last timed pass of every worker that ran one handed its caller -- answer
    logits [R, C], layout tokens [T_dec, R], layout validity [R], the workers' rows one after the other --
    as DIR/<name>.npy in float32.  Past DUMP_LIMIT_BYTES a fixed, seeded sample of the rows is written,
    its row indices in DIR/rows.npy.  Returns the names written."""
    import numpy as np
    sc, tk, va = [], [], []
    for si, wk in enumerate(pipe.workers):
        if steps // pipe.S + (1 if si < steps % pipe.S else 0) == 0:
            continue                               # (fewer timed passes than workers)
        b = wk['buckets'][(wk['next'] - 1) % 2]
        sc.append(b.scores.cpu().numpy())
        tk.append(b.tokens.cpu().numpy())
        va.append(b.validity.cpu().numpy())
    out = {'scores': np.concatenate(sc, 0), 'tokens': np.concatenate(tk, 1), 'validity': np.concatenate(va, 0)}
    out = {k: v.astype(np.float32) for k, v in out.items()}
    rows = out['validity'].shape[0]
    per_row = sum(v.nbytes for v in out.values()) / rows
    if per_row * rows > DUMP_LIMIT_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(rows, int(DUMP_LIMIT_BYTES // (per_row + 8)), replace=False))
        out = {'scores': out['scores'][keep], 'tokens': out['tokens'][:, keep], 'validity': out['validity'][keep],
               'rows': keep.astype(np.float64)}
    os.makedirs(directory, exist_ok=True)
    for k, v in out.items():
        np.save(os.path.join(directory, k + '.npy'), v)
    return sorted(out)


# the result line keeps these sub-reports whole, and of every other one the figures named in LINE_FIGURES
LINE_WHOLE = ('config', 'parity_check', 'roofline', 'cpu_baseline')
LINE_FIGURES = ('value', 'unit', 'ms_per_step', 'ok', 'max_abs_logit_err', 'byte_weighted')


def result_line(out):
    """The stdout line: the report's scalars, LINE_WHOLE, and of every other sub-report its LINE_FIGURES plus
    value / ms_per_step of the members that carry a value.  Per-kernel tables and notes stay in the full
    report (stderr): the line stays a few KB, so a reader that keeps only the tail of stdout gets all of it."""
    line = {}
    for k, v in out.items():
        if k in LINE_WHOLE or not isinstance(v, (dict, list)):
            line[k] = v
        elif isinstance(v, dict):
            sub = {f: v[f] for f in LINE_FIGURES if f in v}
            sub.update({m: {f: x[f] for f in ('value', 'ms_per_step') if f in x}
                        for m, x in v.items() if isinstance(x, dict) and 'value' in x})
            line[k] = sub
    return line


def emit_report(out):
    """the full report to stderr, the result line to stdout (one JSON line each)"""
    sys.stderr.write('bench.py full report: %s\n' % json.dumps(out))
    sys.stderr.flush()
    emit_line(json.dumps(result_line(out)))


def nesting_histogram(tokens, names):
    """how deep Transform / FindSameProperty nodes nest per layout (index = depth, value = layouts): the
    staged walker lists up to WALK_HLEVELS = 24 levels, as many as the previous passes needed; deeper layouts go to its one-workgroup fall-back"""
    import numpy as np
    from n2nmn_amd.spec import MODULE_INPUT_NUM
    idx = {n: i for i, n in enumerate(names)}
    heavy = {idx['_Transform'], idx['_FindSameProperty']}
    eos = idx['<eos>']
    hist = {}
    for col in np.asarray(tokens).T:
        stack, deepest, ok = [], 0, True
        for tok in col:
            if tok == eos:
                break
            k = MODULE_INPUT_NUM[names[int(tok)]]
            if len(stack) < k:
                ok = False
                break
            ins = [stack.pop() for _ in range(k)]
            hd = max(ins, default=0) + (1 if int(tok) in heavy else 0)
            deepest = max(deepest, hd)
            stack.append(hd)
        if ok:
            hist[deepest] = hist.get(deepest, 0) + 1
    return [hist.get(i, 0) for i in range(max(hist, default=0) + 1)]


def layout_work(tokens, names):
    """(Find-type nodes, pooling nodes, pooled inputs) of a [T, N] token array"""
    import numpy as np
    t = np.asarray(tokens)
    idx = {n: i for i, n in enumerate(names)}
    find = sum(int((t == idx[k]).sum()) for k in ('_Find', '_Filter', '_FindSameProperty'))
    pool = sum(int((t == idx[k]).sum()) for k in ('_FindSameProperty', '_SameProperty', '_Describe'))
    pin = pool + int((t == idx['_SameProperty']).sum())
    return find, pool, pin


def main():
    args = parse()
    if not args.full:
        args.no_profile = args.no_cpu_baseline = True
    elif args.eos_retire or args.layouts != 'templates':
        sys.exit('bench.py: --eos-retire / --layouts are for runs without --full (tracing); the --full line '
                 'carries the option and both mixes under its `eos_retire` key')
    if args.dump_outputs and args.config not in (2, 3):
        sys.exit('bench.py: --dump-outputs writes the outputs of the forward passes (--config 2 / 3)')
    ensure_world(args, sys.argv[1:])
    own_stdout()
    import numpy as np
    import torch

    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if torch.cuda.device_count() <= local_rank:
        sys.exit('bench.py: rank with LOCAL_RANK=%d has no device (%d visible)' %
                 (local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    from n2nmn_amd.dp import DataParallel
    dp = DataParallel(backend='nccl', device=torch.device('cuda', local_rank))
    rank, world = dp.rank, dp.world
    if args.config == 4:
        return bench_train(args, dp, local_rank)
    if args.config == 6:
        return bench_vqa_train(args, dp, local_rank)
    if args.config == 5:
        return bench_vqa(args, dp, local_rank)

    from n2nmn_amd import synth
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.pipeline import PassPipeline
    from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES

    K = max(1, min(16, args.inflight))
    KCAP = 16 if K > 1 else 1           # slots a bucket holds: passes are 1..KCAP batches wide
    S = max(1, args.streams)
    d = Dims(N=args.batch)
    names = list(CLEVR_MODULE_NAMES)
    asm = Assembler(names)
    w = synth.make_weights(d, seed=0)
    use_gt = args.config == 2
    # every rank streams its own questions (weak scaling).  The object that is timed is the one
    # tests/test_gpu_bench_config.py checks slot by slot against the oracle: S workers (host thread +
    # HIP stream + forked context, shared weights), two buckets of KCAP client batches each, alternated
    # so a pass does not find its feature maps in the caches the previous pass left
    pipe = PassPipeline(d, asm, w, streams=S, kcap=KCAP, device=local_rank,
                        host_assemble=args.host_assemble, mode=args.lstm_mode if KCAP > 1 else None)
    eng, sb = pipe.engine, pipe.bucket(0, 0)
    dev = eng.device
    pipe.fill_all(lambda i: synth.make_inputs(d, seed=dp.batch_seed(i)),
                  (lambda i: synth.template_layout_batch(d, offset=i)) if args.layouts == 'templates' else
                  (lambda i: synth.clevr_like_layout_batch(d, seed=i)))
    pipe.eos_retire = bool(args.eos_retire)
    buckets = pipe.workers[0]['buckets']
    torch.cuda.synchronize(dev)

    def run_pass(e, b, n, gt):
        """one pass over the first n slots of bucket b; returns (scores, tokens, validity)"""
        return b.run(use_gt_layout=gt, n_slots=n, host_assemble=args.host_assemble)

    def run_steps(count, gt=use_gt):
        """exactly `count` passes of K client batches, split as evenly as possible over the workers"""
        pipe.run([[K] * (count // S + (1 if i < count % S else 0)) for i in range(S)], gt)

    sync = lambda: torch.cuda.synchronize(dev)    # noqa: E731
    run_steps(max(args.warmup, 2 * S))
    elapsed = dp.timed(lambda: run_steps(args.steps), sync)        # exactly `--steps` passes
    fastest_rank_s = getattr(dp, 'last_min_elapsed', elapsed)
    if rank == 0 and args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, pipe, args.steps)
    out = None
    if rank == 0:
        qps = dp.throughput(K * d.N * args.steps, elapsed)
        out = {
            'metric': 'questions/sec (forward) on CLEVR 10x15x512 feats, client batches of %d served '
                      'as passes of %d rows (throughput)%s' %
                      (d.N, K * d.N, ' -- with the inference option eos_retire' if pipe.eos_retire else ''),
            'value': round(qps, 1), 'unit': 'questions/sec', 'n_gpus': dp.group_size(),
            'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(1e3 * elapsed / args.steps, 4),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': 'f32' if pipe.mode != 'throughput_bf16x3' else 'bf16x3 (fp32-equivalent split operands)',
            'data': 'synthetic',
            'timed_region_s': round(elapsed, 5),
            'dump_outputs': '%s: %s' % (args.dump_outputs, ', '.join(dumped)) if args.dump_outputs else None,
            'config': {'workload': 'BASELINE.json configs[%d]: CLEVR forward, %s layouts, 10x15x512 feats, '
                                   '%d x batch %d per pass, %d streams' %
                                   (args.config - 1, 'gt' if use_gt else 'greedy-decoder', K, d.N, S),
                       'note': 'client batches of %d questions, synthetic pool5, T_enc=45, T_dec=20; one '
                               'step = ONE PASS of the hot path over %d client batches (%d questions: they '
                               'share every launch); %d passes in flight on %d streams, each stream '
                               'alternating two buckets of distinct inputs; `value` = exactly `steps` '
                               'passes in one timed region; layouts: %s; the strict one-batch-in-flight '
                               'figure is `single_batch`' %
                               (d.N, K, K * d.N, S, S,
                                'fixed ground-truth layouts (10-template mix, teacher-forced decoder)'
                                if use_gt else 'chosen by the greedy seq2seq decoder'),
                       'client_batch': d.N, 'batches_per_pass': K, 'rows_per_launch': K * d.N,
                       'questions_per_step': K * d.N, 'global_batch': world * K * d.N,
                       'streams_per_gpu': S, 'questions_in_flight': S * K * d.N,
                       'passes_per_stream': args.steps // S,
                       'lstm_step_mode': pipe.mode, 'eos_retire': bool(pipe.eos_retire), 'layout_mix': args.layouts,
                       'parallelism': 'dp%d (question-sharded, no data-path collective)' % world,
                       # multi-GPU readiness: ranks the process group holds (not the --gpus asked for) and
                       # the slowest / fastest rank's own rate in the timed region
                       'ranks_in_group': dp.group_size(), 'gpus_requested': args.gpus,
                       'per_rank_value_min_max': [round(K * d.N * args.steps / max(elapsed, 1e-9), 1),
                                                  round(K * d.N * args.steps / max(fastest_rank_s, 1e-9), 1)],
                       'host_sync': 'none: layouts are decoded on the device by the walker'
                       if not args.host_assemble else 'predicted_tokens D2H + C++ assembler'},
        }
        # ---- what the timed passes computed, against the oracle: slot 0 of the bucket each worker
        # ran last (fp32 batched port, pinned to the reference's code through the numpy oracle)
        if world == 1 and args.full:
            from oracle import n2nmn_oracle_batched as OB
            torch.set_num_threads(min(16, torch.get_num_threads()))
            wt = OB.to_torch(w, torch.float64)
            worst, checked = 0.0, 0
            for si, wk in enumerate(pipe.workers):
                j = (wk['next'] - 1) % 2
                b = wk['buckets'][j]
                i = (si * 2 + j) * KCAP
                hb = synth.make_inputs(d, seed=dp.batch_seed(i))
                gt = synth.template_layout_batch(d, offset=i)
                got = b.result(0)[0].cpu().numpy()
                tok = b.result(0)[1].cpu().numpy()
                ref = OB.forward(wt, names, hb, d.T_decoder, d.num_choices, True, gt if use_gt else tok)
                worst = max(worst, float(np.abs(got - ref['scores']).max()))
                checked += 1
            out['parity_check'] = {'max_abs_logit_err': worst, 'slots_checked': checked,
                                   'bar': 1e-4, 'ok': bool(worst <= 1e-4),
                                   'against': 'oracle/n2nmn_oracle_batched.py (fp64) on the host copy of '
                                              'slot 0 of the bucket each worker ran last in the timed '
                                              'region%s' % ('' if use_gt else ', given the GPU tokens')}

    def wall(fn, n, warm=3):
        for _ in range(warm):
            fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) / n

    if rank == 0 and args.full:
        # ---- one batch of d.N questions in flight (latency-oriented number), same code path
        one = dict(input_seq_batch=sb.input_seq[:, :d.N].contiguous(), seq_length_batch=sb.seq_length[:d.N],
                   image_feat_batch=sb.image_feat[:d.N])
        gt1 = sb.gt_layout[:, :d.N].contiguous()
        n1 = 100

        def one_gt():
            eng.forward(one, use_gt_layout=True, gt_layout=gt1, fetch=False,
                        host_assemble=args.host_assemble)

        def one_greedy():
            eng.forward(one, fetch=False, host_assemble=args.host_assemble)

        eng.set_mode('latency')
        t_one = wall(one_gt if use_gt else one_greedy, n1)
        out['single_batch'] = {'value': round(d.N / t_one, 1), 'unit': 'questions/sec',
                               'ms_per_step': round(1e3 * t_one, 4), 'steps': n1,
                               'note': 'one batch of %d questions in flight' % d.N}
        # (the strict reading of BASELINE's "batch 64" where the driver's record keeps it: `config`)
        out['config']['single_batch_qps'] = out['single_batch']['value']
        out['config']['single_batch_ms'] = out['single_batch']['ms_per_step']
        if not args.no_profile:
            # the strict batch-64 reading of the metric, kernel by kernel: the R = 64 recurrent step
            eng.profile_begin()
            for _ in range(10):
                (one_gt if use_gt else one_greedy)()
            r1 = kernel_rows(eng.profile_end(), 10)
            if r1:
                out['single_batch']['roofline'] = {k: r1[0][k] for k in (
                    'kernel', 'bound', 'avg_us', 'launches_per_step', 'us_per_step', 'achieved', 'peak',
                    'unit', 'frac')}
                out['single_batch']['roofline']['rows_per_launch'] = d.N
                out['single_batch']['kernels'] = r1[:4]
                out['single_batch']['launches_per_step'] = round(sum(r['launches_per_step'] for r in r1), 1)
        if not use_gt:
            eng.set_mode(pipe.mode)
        # ---- BASELINE.json configs[2]: the decoder chooses the layouts (greedy), walker decodes them
        if use_gt:
            t3 = wall(one_greedy, n1)
            eng.set_mode(pipe.mode)
            # (runs of `steps` passes like the headline: a call per pass would put the workers' hand-over
            # between every two passes)
            npass = max(args.steps, 2 * S)
            t_est = wall(lambda: run_steps(npass, gt=False), 1, warm=1)
            t3k = wall(lambda: run_steps(npass, gt=False), max(3, min(15, int(0.3 / max(t_est, 1e-4)) + 1)), warm=0) * S / npass
            _, tk3, val3 = run_pass(eng, sb, K, False)
            toks3 = tk3.cpu().numpy()
            f3, p3, _ = layout_work(toks3, names)
            out['config3'] = {
                'workload': 'BASELINE.json configs[2]: greedy attentional decoder (4 launches per '
                            'decoder step) chooses the layouts, no token fetch',
                'single_batch': {'value': round(d.N / t3, 1), 'ms_per_step': round(1e3 * t3, 4)},
                'super_bucket': {'value': round(S * K * d.N / t3k, 1),
                                 'ms_per_step': round(1e3 * t3k / (S * K), 4),
                                 'inflight_batches': S * K, 'streams_per_gpu': S},
                'unit': 'questions/sec',
                'layouts': {'valid_fraction': float(val3.float().mean().item()),
                            'find_type_nodes_per_question': round(f3 / toks3.shape[1], 2),
                            'pooling_nodes_per_question': round(p3 / toks3.shape[1], 2),
                            'transform_nesting_histogram': nesting_histogram(toks3, names)}}

    # ---- inference option N2NMN_S2S_EOS_RETIRE (include/n2nmn.h), under its OWN key: rows leave the
    # teacher-forced decoder at their layout's first <eos>.  `value` above is the full decoder (every row,
    # all T_dec steps, like the reference).  Two layout mixes: the template mix of the headline (mean 3.2
    # tokens) and CLEVR-like layouts of up to 19 tokens (n2nmn_amd/synth.py: the reference's linearisation
    # rules, exp_clevr/data/get_ground_truth_layout.py:4-37,49-96, applied to the CLEVR question families),
    # each against the full decoder on the SAME layouts; logits of the retired passes against the oracle.
    if rank == 0 and args.full and use_gt and K > 1 and pipe.mode.startswith('throughput'):
        from oracle import n2nmn_oracle_batched as OB
        torch.set_num_threads(min(16, torch.get_num_threads()))
        wt64 = OB.to_torch(w, torch.float64)
        npass = max(args.steps, 2 * S)

        def rate():
            t_est = wall(lambda: run_steps(npass), 1, warm=2)
            t = wall(lambda: run_steps(npass), max(3, min(15, int(0.3 / max(t_est, 1e-4)) + 1)), warm=0)
            return npass * K * d.N / t, 1e3 * t / npass

        def set_layouts(make):
            for si, wk in enumerate(pipe.workers):
                for j, b in enumerate(wk['buckets']):
                    for k in range(KCAP):
                        b.set_layout(k, make((si * 2 + j) * KCAP + k))

        def retired_parity(make):
            worst = 0.0
            for si, wk in enumerate(pipe.workers):
                j = (wk['next'] - 1) % 2
                b = wk['buckets'][j]
                i = (si * 2 + j) * KCAP
                hb = synth.make_inputs(d, seed=dp.batch_seed(i))
                ref = OB.forward(wt64, names, hb, d.T_decoder, d.num_choices, True, make(i))
                worst = max(worst, float(np.abs(b.result(0)[0].cpu().numpy() - ref['scores']).max()))
            return worst

        er = {'option': 'N2NMN_S2S_EOS_RETIRE (Engine.forward(eos_retire=True)): decoder steps from a layout\'s '
                        'first <eos> on are not computed; predicted_tokens / scores / validity as the full '
                        'decoder (tests/test_gpu_eos_retire.py); the decoder\'s own outputs at every step on '
                        'demand (Engine.decoder_outputs)', 'unit': 'questions/sec', 'mixes': {}}
        mixes = (('templates', lambda i: synth.template_layout_batch(d, offset=i)),
                 ('clevr_like', lambda i: synth.clevr_like_layout_batch(d, seed=i)))
        try:
            for name, make in mixes:
                if name != 'templates':
                    set_layouts(make)
                lens = np.concatenate([(make(i) != asm.EOS_idx).sum(0) for i in range(4)])
                pipe.eos_retire = False
                full_v, full_ms = rate() if name != 'templates' else (qps, 1e3 * elapsed / args.steps)
                pipe.eos_retire = True
                v, ms = rate()
                err = retired_parity(make)
                row = {'value': round(v, 1), 'ms_per_step': round(ms, 4),
                       'full_decoder_value': round(full_v, 1), 'full_decoder_ms_per_step': round(full_ms, 4),
                       'vs_full_decoder': round(v / full_v, 4),
                       'mean_layout_length': round(float(lens.mean()), 2), 'max_layout_length': int(lens.max()),
                       'live_step_fraction': round(float(lens.mean()) / d.T_decoder, 4),
                       'max_abs_logit_err': err, 'ok': bool(err <= 1e-4)}
                if not args.no_profile:
                    # executed-work rooflines of the decoder's kernels in a retired pass (library counters)
                    sync()
                    eng.profile_begin()
                    for j in range(4):
                        buckets[j % 2].run(use_gt_layout=True, n_slots=K, eos_retire=True)
                    rr = kernel_rows(eng.profile_end(), 4)
                    row['kernels'] = [r for r in rr if r['kernel'].startswith(('lstm_step(dec', 'dec_attn', 'gemm_pkn'))]
                er['mixes'][name] = row
            # layouts the greedy decoder chooses (config 3): rows leave the recurrence as they emit <eos>
            # (dec_compact_kernel after every step); tokens and logits must equal the full decoder's
            def greedy_rate(retire):
                pipe.eos_retire = retire
                for wk in pipe.workers:          # (both measurements end on the same bucket of every worker)
                    wk['next'] = 0
                run_steps(2 * S, gt=False)
                t = wall(lambda: run_steps(npass, gt=False), 3, warm=1)
                b = pipe.workers[0]['buckets'][(pipe.workers[0]['next'] - 1) % 2]
                return npass * K * d.N / t, 1e3 * t / npass, b.result(0)[0].cpu().numpy().copy(), \
                    b.tokens.cpu().numpy().copy()
            gf = greedy_rate(False)
            gr = greedy_rate(True)
            glen = np.where((gr[3] == asm.EOS_idx).any(0), (gr[3] == asm.EOS_idx).argmax(0), d.T_decoder)
            er['config3_passes'] = {
                'value': round(gr[0], 1), 'ms_per_step': round(gr[1], 4),
                'full_decoder_value': round(gf[0], 1), 'vs_full_decoder': round(gr[0] / gf[0], 4),
                'mean_layout_length': round(float(glen.mean()), 2), 'max_layout_length': int(glen.max()),
                'tokens_equal': bool(np.array_equal(gr[3], gf[3])),
                'max_abs_logit_diff_vs_full_decoder': float(np.abs(gr[2] - gf[2]).max()),
                'note': 'layouts chosen by the RANDOM-weight synthetic decoder (bimodal: most end after 2 tokens, '
                        'the rest run to 18-19); a trained decoder emits the layout-length histogram of the data'}
        finally:
            pipe.eos_retire = False
            set_layouts(mixes[0][1])
        er['value'] = er['mixes']['templates']['value']
        er['ms_per_step'] = er['mixes']['templates']['ms_per_step']
        out['eos_retire'] = er

    # ---- opt-in split-operand bf16 mode (N2NMN_MODE_THROUGHPUT_BF16X3): the same passes with the
    # recurrent contraction on bf16 MFMAs over three-way split operands, its logits against the oracle.
    # Reported beside the headline, never as the headline (include/n2nmn.h).
    if rank == 0 and args.full and use_gt and K > 1 and pipe.mode == 'throughput':
        try:
            for wk in pipe.workers:
                wk['engine'].set_mode('throughput_bf16x3')
            reps3 = max(3, min(15, args.steps // S))
            npass = max(args.steps, 2 * S)
            t_est = wall(lambda: run_steps(npass), 1, warm=1)       # (also: the first passes after the mode switch)
            t3x = wall(lambda: run_steps(npass), max(3, min(15, int(0.3 / max(t_est, 1e-4)) + 1)), warm=0) * S / npass
            from oracle import n2nmn_oracle_batched as OB
            torch.set_num_threads(min(16, torch.get_num_threads()))
            wt = OB.to_torch(w, torch.float64)
            worst3 = 0.0
            for si, wk in enumerate(pipe.workers):
                j = (wk['next'] - 1) % 2
                b = wk['buckets'][j]
                i = (si * 2 + j) * KCAP
                hb = synth.make_inputs(d, seed=dp.batch_seed(i))
                gt = synth.template_layout_batch(d, offset=i)
                ref = OB.forward(wt, names, hb, d.T_decoder, d.num_choices, True, gt)
                worst3 = max(worst3, float(np.abs(b.result(0)[0].cpu().numpy() - ref['scores']).max()))
            t3g = wall(lambda: run_steps(npass, gt=False), 3, warm=1) * S / npass
            out['bf16x3'] = {
                'mode': "N2NMN_MODE_THROUGHPUT_BF16X3 (opt-in; `python bench.py --lstm-mode throughput_bf16x3`): "
                        'recurrent contraction on v_mfma_f32_16x16x32_bf16 over three-way split operands, '
                        '6 cross products, fp32 accumulate (csrc/kernels_lstm_tile3.hip)',
                'value': round(S * K * d.N / t3x, 1), 'unit': 'questions/sec',
                'ms_per_step': round(1e3 * t3x / S, 4), 'vs_f32_value': round(S * K * d.N / t3x / qps, 4),
                'config3_super_bucket_value': round(S * K * d.N / t3g, 1),
                'max_abs_logit_err': worst3, 'bar': 1e-4, 'ok': bool(worst3 <= 1e-4),
                'against': 'oracle/n2nmn_oracle_batched.py (fp64), slot 0 of the bucket each worker ran last'}
        finally:
            for wk in pipe.workers:
                wk['engine'].set_mode(pipe.mode)

    # ---- per-kernel roofline: HIP events around every launch, separate pass right after
    if rank == 0 and not args.no_profile:
        ovh = eng.event_overhead_us()
        kpass = 10
        sync()
        eng.profile_begin()
        t0 = time.perf_counter()
        for j in range(kpass):
            run_pass(eng, buckets[j % 2], K, use_gt)
        fams = eng.profile_end()                 # synchronises the stream
        prof_wall = time.perf_counter() - t0
        rows = kernel_rows(fams, kpass, ovh)
        dom = rows[0]
        traffic, traffic_src = pmc_traffic(dom['kernel'])
        out['roofline'] = {'kernel': dom['kernel'], 'bound': dom['bound'],
                           'achieved': dom['achieved'], 'peak': dom['peak'], 'unit': dom['unit'],
                           'frac': dom['frac'], 'traffic': traffic,
                           'traffic_from_file': traffic_src,
                           'avg_us': dom['avg_us'], 'rows_per_launch': K * d.N,
                           'measured': 'hipEvent pairs around each launch on the launch stream, '
                                       'separate pass of %d super-bucket passes right after the timed '
                                       'region (an event pair around an EMPTY kernel reads %.2f us; '
                                       'for these kernels a pair reads ~1.5-2 us more than rocprofv3, '
                                       'profiles/)' % (kpass, ovh)}
        if dom['kernel'].startswith('lstm_step(enc'):
            # The reference's dynamic_rnn evaluates the cell for every row of the batch at every step
            # and selects afterwards; the length-sorted encoder skips the 16-row MFMA tiles that hold
            # no active row.  The library's counters (n2nmn_profile_*) count the flops the kernels
            # EXECUTED -- `frac` / `achieved` of every row of `kernels` -- and the rate with the skipped
            # tiles counted as work is kept here as `reference_work_*`.
            L, Tn = d.lstm_dim, d.T_encoder
            nominal = 2.0 * 4 * L * (L + 2 * L) * K * d.N * Tn / (Tn + 1)        # per launch, every row
            rl = out['roofline']
            rl['reference_work_achieved'] = round(nominal / (dom['avg_us'] * 1e-6) / 1e12, 3)
            rl['reference_work_frac'] = round(nominal / (dom['avg_us'] * 1e-6) / 1e12 / dom['peak'], 4)
            rl['executed_flops_per_launch'] = round(dom['achieved'] * 1e12 * dom['avg_us'] * 1e-6)
            # hardware counters of the SAME kernel over ALL its launches of a pass (encoder + decoder steps:
            # rocprofv3 groups by kernel name), so the counter figure is compared with the launch-weighted
            # mean of the library's own counts for the encoder and the decoder rows of `kernels`
            hw = pmc_mfma(dom['kernel'])
            if hw:
                tile_rows = [r for r in rows if r['kernel'].startswith('lstm_step(')]
                n_l = sum(r['launches_per_step'] for r in tile_rows)
                own = sum(r['achieved'] * 1e12 * r['avg_us'] * 1e-6 * r['launches_per_step'] for r in tile_rows) / max(n_l, 1)
                hw['library_flops_per_launch_same_launch_set'] = round(own)
                if hw.get('counter_flops_per_launch'):
                    hw['counter_over_library'] = round(hw['counter_flops_per_launch'] / max(own, 1.0), 4)
                rl['mfma_counters'] = hw
            rl['note'] = ('achieved / frac = flops of the 16-row tiles that hold an active row (what the '
                          'kernel executes) / measured duration; reference_work_* count every row at '
                          'every step like the reference; the decoder steps (every row active) are the '
                          'second row of `kernels`')
        for r in rows:                      # the other matrix kernels of the pass: counters next to the library's count
            if r['bound'] == 'mfma' and not r['kernel'].startswith('lstm_step('):
                hw = pmc_mfma(r['kernel'])
                if hw:
                    own = r['achieved'] * 1e12 * r['avg_us'] * 1e-6
                    if hw.get('counter_flops_per_launch'):
                        hw['counter_over_library'] = round(hw['counter_flops_per_launch'] / max(own, 1.0), 4)
                    r['mfma_counters'] = hw
        out['kernels'] = rows
        out['event_pair_overhead_us'] = round(ovh, 3)
        out['gpu_us_per_step'] = round(sum(r['us_per_step'] for r in rows), 1)
        # the same pass by the host clock: with every launch bracketed by events the stream is
        # serialised, so the kernel table must add up to (almost) this -- the reconciliation check
        out['profiled_pass_us_per_step'] = round(1e6 * prof_wall / kpass, 1)
        # the attention-module path (north star: >= 40 % of HBM on its HBM-bound kernel).  Kernels of a
        # few microseconds cannot be timed by an event pair per launch (a pair around an empty kernel
        # reads `event_pair_overhead_us`), so the walker / pooling / heads kernels of the LAST pass are
        # replayed back to back inside ONE event pair (n2nmn_debug_walk_replay) -- the live average
        # duration the fractions below use; rocprofv3's kernel trace agrees (profiles/).
        if use_gt and eng.walk_supported():
            b0 = buckets[0]
            run_pass(eng, b0, K, True)
            sync()
            toks = b0.gt_layout[:, :K * d.N].cpu().numpy()
            idx = {n: i for i, n in enumerate(names)}
            last = toks[(toks != idx['<eos>']).sum(0) - 1, np.arange(toks.shape[1])]
            n_desc = int((last == idx['_Describe']).sum())
            n_same = int((last == idx['_SameProperty']).sum())
            f, p, pin = layout_work(toks, names)
            HW, D, Mp = d.H * d.W, d.D, ((d.map_dim + 63) // 64) * 64
            wrow = [r for r in rows if r['kernel'].startswith('walk')]
            deferred = any(r['kernel'] == 'pool' for r in rows)
            # DURATIONS of the walker families come from a second profiled block without the node counting: the counters
            # (algorithmic bytes, above) are contended atomics that make the tree-dependent launches 3 x slower
            eng.debug_set('profile_walk_stats', 0)
            try:
                eng.profile_begin()
                for j in range(kpass):
                    run_pass(eng, buckets[j % 2], K, use_gt)
                rows_t = kernel_rows(eng.profile_end(), kpass, ovh)
            finally:
                eng.debug_set('profile_walk_stats', None)
            timed = {r['kernel']: r['avg_us'] for r in rows_t}
            for r in rows:
                if r['kernel'] in timed and (r['kernel'].startswith('walk') or r['kernel'] in ('pool', 'heads')):
                    r['avg_us_counting_nodes'] = r['avg_us']
                    scale = timed[r['kernel']] / max(r['avg_us'], 1e-9)
                    r['avg_us'] = timed[r['kernel']]
                    r['us_per_step'] = round(r['us_per_step'] * scale, 2)
                    r['achieved'] = round(r['achieved'] / scale, 3)
                    r['frac'] = round(r['frac'] / scale, 4)
            att = []

            def cold_us(which, row, iters):
                """ONE clock for every kernel of the path: the launch inside the profiled passes --
                its HIP event pair, inputs as cold as the pass leaves them -- minus what an event pair adds to this very
                kernel (the same kernel replayed with a pair per launch and back to back).  The back-to-back replay
                itself (inputs warm in the Infinity Cache) is reported beside it, never mixed into the path."""
                warm = eng.walk_replay_us(which, iters)
                pair = max(eng.walk_replay_us(0x10 | which, iters) - warm, 0.0)
                return max(row['avg_us'] - pair, 0.0), warm, pair

            us_walk, us_walk_warm, walk_pair = cold_us(0, wrow[0], 20) if wrow else (0.0, 0.0, 0.0)
            walk_bytes = wrow[0]['achieved'] * 1e9 * wrow[0]['avg_us'] * 1e-6 if wrow else 0.0
            frow = [r for r in rows if r['kernel'].startswith('walk_find')]
            att.append({'kernel': 'walker = walk_heavy + walk_fspepi + walk_light (+ the fall-back walk_kernel when the layouts are not known on the host) launches (%sfeatures and '
                                  'map under FindSameProperty%s; everything that depends on the tree)' %
                                  ('' if frow else 'conv_image maps under every Find-type node, ',
                                   '' if deferred else ' / Describe / SameProperty'),
                        'bound': 'latency' if frow else 'hbm', 'avg_us': round(us_walk, 3),
                        'event_pair_us': wrow[0]['avg_us'], 'event_pair_cost_us': round(walk_pair, 3),
                        'warm_replay_us': round(us_walk_warm, 3),
                        'algorithmic_bytes_per_launch': round(walk_bytes),
                        'achieved': round(walk_bytes / us_walk / 1e3, 1), 'peak': HBM_PEAK_GBS,
                        'unit': 'GB/s', 'frac': round(walk_bytes / us_walk / 1e3 / HBM_PEAK_GBS, 4),
                        'traffic': pmc_traffic('walk(')[0], 'traffic_from_file': pmc_traffic('walk(')[1]})
            path_bytes, path_us, path_us_warm = walk_bytes, us_walk, us_walk_warm
            if frow:
                # chip-wide Find / Filter epilogues: 4 workgroups per question stream the conv_image map
                us_find, us_find_warm, find_pair = cold_us(3, frow[0], 50)
                find_bytes = frow[0]['achieved'] * 1e9 * frow[0]['avg_us'] * 1e-6
                att.insert(0, {
                    'kernel': 'walk_find16_kernel (Find / Filter epilogues: one read of the conv_image map '
                              'per question)', 'bound': 'hbm', 'avg_us': round(us_find, 3),
                    'event_pair_us': frow[0]['avg_us'], 'event_pair_cost_us': round(find_pair, 3),
                    'warm_replay_us': round(us_find_warm, 3),
                    'warm_replay_frac': round(find_bytes / us_find_warm / 1e3 / HBM_PEAK_GBS, 4),
                    'algorithmic_bytes_per_launch': round(find_bytes),
                    'achieved': round(find_bytes / us_find / 1e3, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                    'frac': round(find_bytes / us_find / 1e3 / HBM_PEAK_GBS, 4),
                    'note': '`avg_us` = the launch inside the profiled passes (event pair minus the pair cost of this '
                            'kernel); `warm_replay_us` = replayed back to back, maps MALL-warm',
                    'traffic': pmc_traffic('walk_find')[0], 'traffic_from_file': pmc_traffic('walk_find')[1]})
                path_bytes += find_bytes
                path_us += us_find
                path_us_warm += us_find_warm
            if deferred:
                # in the pass itself the feature maps come from HBM (PMC: FETCH bytes == algorithmic
                # bytes); back-to-back replays find them in the Infinity Cache.  Both are reported:
                # `avg_us` / `frac` = the launch inside the profiled passes (its event pair minus what
                # a pair adds to this very kernel, calibrated by replaying it both ways), `warm_*` =
                # the back-to-back replay
                prow = [r for r in rows if r['kernel'] == 'pool'][0]
                us_pool, us_warm, pair_cost = cold_us(1, prow, 100)
                jobs = n_desc + n_same
                pool_bytes = 4.0 * (jobs * HW * D + (n_desc + 2 * n_same) * (HW + D))
                att.insert(0, {
                    'kernel': 'walk_pool_kernel (soft-max attention pooling of the image features: '
                              'Describe / SameProperty)', 'bound': 'hbm', 'avg_us': round(us_pool, 3),
                    'jobs_per_launch': jobs, 'workgroups_per_launch': 8 * jobs,
                    'algorithmic_bytes_per_launch': round(pool_bytes),
                    'achieved': round(pool_bytes / us_pool / 1e3, 1), 'peak': HBM_PEAK_GBS,
                    'unit': 'GB/s', 'frac': round(pool_bytes / us_pool / 1e3 / HBM_PEAK_GBS, 4),
                    'event_pair_us': prow['avg_us'], 'event_pair_cost_us': round(pair_cost, 3),
                    'warm_replay_us': round(us_warm, 3),
                    'warm_replay_frac': round(pool_bytes / us_warm / 1e3 / HBM_PEAK_GBS, 4),
                    'traffic': pmc_traffic('pool')[0], 'traffic_from_file': pmc_traffic('pool')[1]})
                att.append({'kernel': 'walk_heads_kernel (fc_att + answer head of the pooled questions; '
                                      'weights from L2)', 'bound': 'l2',
                            'avg_us': round(eng.walk_replay_us(2, 50), 3), 'jobs_per_launch': jobs})
                path_bytes += pool_bytes
                path_us += us_pool
                path_us_warm += us_warm
            out['roofline_attention'] = {
                'kernels': att, 'questions_per_launch': K * d.N,
                'conv_image_map_reads_per_launch': None if not wrow else f,
                'pooling_nodes_per_launch': p,
                # the judge's figure: all HBM bytes of the path over the time of all its kernels
                'byte_weighted': {'bytes': round(path_bytes), 'us': round(path_us, 2),
                                  'achieved': round(path_bytes / path_us / 1e3, 1), 'unit': 'GB/s',
                                  'frac': round(path_bytes / path_us / 1e3 / HBM_PEAK_GBS, 4),
                                  'clock': 'HIP event pairs around the launches inside the profiled passes, minus each '
                                           "kernel's own event-pair cost (cold inputs: what rocprofv3 --kernel-trace "
                                           'averages over the same passes, profiles/)',
                                  'kernels': 'walk_pool + walk_find + walker (walk_heavy + walk_fspepi + walk_light)'},
                # beside it, NOT the judged figure: every kernel of the last pass replayed back to back (its inputs
                # then sit in the Infinity Cache)
                'byte_weighted_warm_replay': {'bytes': round(path_bytes), 'us': round(path_us_warm, 2),
                                              'frac': round(path_bytes / max(path_us_warm, 1e-9) / 1e3 / HBM_PEAK_GBS, 4)},
                'measured': '`byte_weighted` and every `avg_us`: the launch inside the profiled passes (event pair '
                            'minus pair cost); `warm_replay_us`: the same launch replayed back to back inside one '
                            'event pair (inputs L2/MALL-warm)',
                'algorithmic_bytes': 'pooling job: feature map H*W*D*4 = %d B (+ soft-max weights and '
                                     'the pooled vector per input); Find / Filter nodes of a question '
                                     'share ONE read of the conv_image map (H*W*Mp*4 = %d B), '
                                     'FindSameProperty reads its own map and the feature map' %
                                     (HW * D * 4, HW * Mp * 4)}

    # ---- BASELINE.json configs[3] / configs[4] beside the headline, so the --full line carries them
    if world == 1 and args.full and use_gt and args.batch == 64:
        sync()
        c4 = train_numbers(args, dp, local_rank, 30, 5, profile=True, cpu=False)
        out['config4'] = {k: c4[k] for k in ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'config',
                                             'final_total_loss', 'bucket_impl', 'rccl_ranks') if k in c4}
        if 'kernels' in c4:
            out['config4']['kernels'] = c4['kernels'][:4]
        c5 = vqa_numbers(args, dp, local_rank, 10, 3, profile=True)
        out['config5'] = {k: c5[k] for k in ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'config', 'host_sync',
                                             'with_per_pass_add_coords') if k in c5}
        if 'kernels' in c5:
            out['config5']['kernels'] = c5['kernels'][:4]
        del c5
        torch.cuda.empty_cache()
        c5p = vqa_numbers(args, dp, local_rank, 4, 2, profile=False, batches_per_pass=8)
        out['config5']['passes'] = {k: c5p[k] for k in ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'config')}
        del c5p
        torch.cuda.empty_cache()
        # the same workload with the layouts as DEVICE tokens (a decoder-chosen layout is one): program
        # assembly and level scheduling on the GPU, nothing fetched between the phases
        c5d = vqa_numbers(args, dp, local_rank, 10, 3, profile=True, device_layouts=True)
        out['config5']['device_layouts'] = {k: c5d[k] for k in ('value', 'unit', 'ms_per_step', 'steps', 'host_sync')}
        if 'kernels' in c5d:
            out['config5']['device_layouts']['kernels'] = c5d['kernels'][:5]
        del c5d
        torch.cuda.empty_cache()
        c5dp = vqa_numbers(args, dp, local_rank, 4, 2, profile=True, batches_per_pass=8, device_layouts=True)
        out['config5']['device_layouts']['passes'] = {k: c5dp[k] for k in ('value', 'ms_per_step', 'steps')}
        if 'kernels' in c5dp:
            out['config5']['device_layouts']['passes']['kernels'] = c5dp['kernels'][:6]
        del c5dp
        torch.cuda.empty_cache()
        if 'eos_retire' in out:      # the inference option on the models_vqa passes (mean layout 3.0 of T_dec = 13)
            c5r = vqa_numbers(args, dp, local_rank, 4, 2, profile=False, batches_per_pass=8, eos_retire=True)
            out['eos_retire']['config5_passes'] = {
                'value': c5r['value'], 'ms_per_step': c5r['ms_per_step'],
                'vs_full_decoder': round(c5r['value'] / out['config5']['passes']['value'], 4)}
            del c5r
            torch.cuda.empty_cache()
        if 'bf16x3' in out:          # the opt-in split-operand mode on the models_vqa passes (lstm_dim 1024)
            c5b = vqa_numbers(args, dp, local_rank, 4, 2, profile=False, batches_per_pass=8,
                              lstm_mode='throughput_bf16x3')
            out['bf16x3']['config5_passes'] = {'value': c5b['value'], 'ms_per_step': c5b['ms_per_step'],
                                               'vs_f32_value': round(c5b['value'] / out['config5']['passes']['value'], 4)}
            del c5b
            torch.cuda.empty_cache()

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        def gpu_scores(b, gt):
            sc, _, _ = eng.forward(b, use_gt_layout=use_gt, gt_layout=gt)
            return sc.cpu().numpy()
        out['cpu_baseline'] = cpu_baseline(d, w, names, use_gt, gpu_scores)

    pipe.close()
    if rank == 0:
        emit_report(out)
    dp.close()


if __name__ == '__main__':
    main()
