#!/usr/bin/env python3
"""Step time of ShapesTrainer.step (exp_shapes/train_shapes_gt_layout.py geometry: N = 256, T_enc 15, T_dec 11,
lstm_dim 256, encoder / decoder dropout on) from device events: median over --steps steps after --warmup.
Batch: the 12 dataset questions of tests/golden/shapes_golden.json tiled to N (the images with noise).

    python tools/shapes_train_step_time.py [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--N', type=int, default=256)
    a = ap.parse_args()
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
