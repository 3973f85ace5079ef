#!/usr/bin/env python3
"""Step time of ShapesTrainer.step (exp_shapes/train_shapes_gt_layout.py geometry: N = 256, T_enc 15, T_dec 11,
lstm_dim 256, encoder / decoder dropout on) from device events: median over --steps steps after --warmup.
Batch: the 12 dataset questions of tests/golden/shapes_golden.json tiled to N (the images with noise).

    python tools/shapes_train_step_time.py [--steps 50] [--warmup 10]

--rl: the from-scratch step of exp_shapes/train_shapes_scratch.py (T_dec 7) in ONE session, three legs on the same
batch: the single-pass ShapesTrainer.step_rl (n2nmn_train_sample, then the module network), the two-pass form
(Engine.seq2seq samples, forward_backward(objective=1) repeats encoder and decoder teacher-forced) and the cloning
step ShapesTrainer.step as the yardstick.  The token fetch is inside the timed step: it is part of the algorithm.
Each leg: --runs runs of --steps steps after --warmup warm-up steps, the legs alternating run by run; reported
per leg: the median over runs of the run's median step, with the spread of the run medians.

    python tools/shapes_train_step_time.py --rl --runs 5 --steps 200 --warmup 50
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def main_rl(a):
    import torch
    import float_cases as FC
    from n2nmn_amd.models_shapes import ShapesTrainer, shapes_engine
    Td = 7
    d, batch, gt, w, nv_txt, _ = FC.shapes_setup()
    with open(os.path.join(ROOT, 'tests', 'golden', 'shapes_golden.json')) as f:
        labels = np.array(json.load(f)['labels'], np.int32)
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 12, size=a.N)
    img = batch['image_batch'][idx] + rng.standard_normal((a.N,) + batch['image_batch'].shape[1:])
    b = dict(image_batch=img.astype(np.float32), input_seq_batch=batch['text_seq_batch'][:, idx],
             seq_length_batch=batch['seq_length_batch'][idx], answer_label_batch=labels[idx])
    g = np.ascontiguousarray(gt[:Td, idx])          # (every dataset layout ends inside 7 steps)
    assert (g[-1] == 4).all()
    w32 = {k: np.asarray(v, np.float32) for k, v in w.items()}
    T = b['input_seq_batch'].shape[0]
    # inputs live on the device, as a data feeder leaves them; the uniforms come from a device generator
    trs = {}
    for leg in ('single_pass', 'two_pass', 'cloning'):
        tr = ShapesTrainer(shapes_engine(nv_txt, N=a.N, T_decoder=Td))
        tr.load_weights(w32)
        trs[leg] = tr
    dev = trs['cloning'].engine.device
    bd = {k: torch.as_tensor(v).to(dev) for k, v in b.items()}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def step(leg):
        tr = trs[leg]
        if leg == 'cloning':
            tr.step(bd, g)
            return
        u = torch.rand((Td, a.N), generator=gen, device=dev)
        if leg == 'single_pass':
            tr.step_rl(bd, u)
            return
        mult = tr.multipliers(T, a.N, Td, None)
        s2s = tr.engine.seq2seq(bd['input_seq_batch'], bd['seq_length_batch'], Td, sample_uniforms=u,
                                dropout=(mult.get('enc0'), mult.get('dec0')))
        tok = s2s['predicted_tokens'].cpu().numpy()
        seen = np.cumsum(tok == 4, axis=0) > 0
        tok[1:][seen[:-1]] = 4                       # the <eos> latch on the fetched tokens
        scale = tr._forward_backward(bd, tok, True, 1, mult=mult)
        tr.apply(scale)

    for leg in trs:
        for _ in range(a.warmup):
            step(leg)
    torch.cuda.synchronize()
    runs = {leg: [] for leg in trs}
    for _ in range(a.runs):
        for leg in trs:
            times = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(leg)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            runs[leg].append(float(np.median(times)))
    out = dict(metric='shapes_train_rl_step_ms', N=a.N, T_enc=T, T_dec=Td, dropout=True, runs=a.runs,
               steps=a.steps, warmup=a.warmup)
    for leg, r in runs.items():
        out[leg] = dict(median_ms=float(np.median(r)), min_ms=float(np.min(r)), max_ms=float(np.max(r)), runs_ms=r)
        assert np.isfinite(trs[leg].losses.cpu().numpy()[:5]).all()
    out['validity_single_pass'] = float(np.mean(trs['single_pass'].last_validity))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--N', type=int, default=256)
    ap.add_argument('--rl', action='store_true')
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    if a.rl:
        return main_rl(a)
    import torch
    import float_cases as FC
    from n2nmn_amd.models_shapes import ShapesTrainer, shapes_engine
    d, batch, gt, w, nv_txt, _ = FC.shapes_setup()
    with open(os.path.join(ROOT, 'tests', 'golden', 'shapes_golden.json')) as f:
        labels = np.array(json.load(f)['labels'], np.int32)
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 12, size=a.N)
    img = batch['image_batch'][idx] + rng.standard_normal((a.N,) + batch['image_batch'].shape[1:])
    b = dict(image_batch=img.astype(np.float32), input_seq_batch=batch['text_seq_batch'][:, idx],
             seq_length_batch=batch['seq_length_batch'][idx], answer_label_batch=labels[idx])
    g = np.ascontiguousarray(gt[:, idx])
    tr = ShapesTrainer(shapes_engine(nv_txt, N=a.N))
    tr.load_weights({k: np.asarray(v, np.float32) for k, v in w.items()})
    for _ in range(a.warmup):
        tr.step(b, g)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses = tr.step(b, g)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    l = losses.cpu().numpy()[:4]
    print(json.dumps(dict(metric='shapes_train_step_ms', N=a.N, dropout=True, steps=a.steps, warmup=a.warmup,
                          median_ms=float(np.median(times)), min_ms=float(np.min(times)),
                          p90_ms=float(np.percentile(times, 90)), losses=[float(x) for x in l])))
    assert np.isfinite(l).all()


if __name__ == '__main__':
    main()
