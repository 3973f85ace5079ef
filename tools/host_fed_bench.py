#!/usr/bin/env python3
"""PCIe-inclusive throughput: the bench's super-bucket pipeline (2 buckets x 8 batches of 64) with
every batch's inputs (19.7 MB of features + text) copied from PINNED HOST memory into its slot on a
copy stream, under the other bucket's compute.  bench.py's `value` has the inputs resident in HBM;
this is the rate when they are not.

The compact feed (include/n2nmn.h section 11) ships less:
    --feat-dtype float16        the features cross the link as IEEE halves
    --questions-per-image Q     one feature row per image, Q consecutive questions share it (CLEVR ~10, VQA ~5)
and n2nmn_features_expand widens / gathers them into the slot on the copy stream, behind the copy.  The defaults
(float32, Q = 1) are the plain run: the same copies into the slots as before the options existed.
    --variant vqa               models_vqa at batch 128: features through VQAEngine.fill_slab into two slabs
    --expand-only               only the expand kernel alone (fp16 -> fp32), cold, at the size of a 1024-row CLEVR pass,
                                beside the runtime's device-to-device copy of the same fp32 destination (also printed
                                after a CLEVR run with a compact feed)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compact_rows(feat, half, Q):
    """[N, H, W, D] float32 -> (rows [ceil(N / Q), H, W, D] in the container dtype, index int32 [N] or None)"""
    n = feat.shape[0]
    index = None
    if Q > 1:
        index = (np.arange(n) // Q).astype(np.int32)
        feat = feat[:(n + Q - 1) // Q]
    return np.ascontiguousarray(feat.astype(np.float16) if half else feat), index


def expand_alone(dev, half=True, rows=1024, reps=10):
    """cold: between timed launches a 1 GiB fill evicts source and destination from L2 and the Infinity Cache"""
    import torch
    from n2nmn_amd import feed
    from n2nmn_amd.spec import Dims
    d = Dims()
    src = torch.randn((rows, d.H, d.W, d.D), device=dev).to(torch.float16 if half else torch.float32)
    dst = torch.empty((rows, d.H, d.W, d.D), dtype=torch.float32, device=dev)
    other = torch.randn((rows, d.H, d.W, d.D), device=dev)
    index = torch.arange(rows, dtype=torch.int32, device=dev)
    evict = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    runs = {'expand': lambda: feed.expand(src, None, dst),
            'expand, identity index': lambda: feed.expand(src, index, dst),
            'device-to-device copy': lambda: dst.copy_(other)}
    ms = {k: [] for k in runs}
    for rep in range(reps + 2):
        for k, fn in runs.items():                     # alternating, so drift hits all alike
            evict.fill_(float(rep))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                ms[k].append(e0.elapsed_time(e1))
    out_b = dst.numel() * 4
    for k, v in ms.items():
        in_b = out_b if k.startswith('device') else src.numel() * src.element_size()
        med = float(np.median(v))
        print('expand alone, cold, %d rows %s -> float32: %-24s median %.3f ms (min %.3f, max %.3f), %.2f TB/s read + written'
              % (rows, str(src.dtype).split('.')[-1], k, med, min(v), max(v), (in_b + out_b) / med / 1e9))


def clevr(a):
    import torch
    from n2nmn_amd import feed, synth
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
    from n2nmn_amd.superbucket import SuperBucket
    K, passes = 8, a.passes
    half, Q = a.feat_dtype == 'float16', a.questions_per_image
    compact = half or Q > 1
    d = Dims()
    asm = Assembler(list(CLEVR_MODULE_NAMES))
    w = synth.make_weights(d, seed=0)
    buckets = [SuperBucket(d, asm, K=K) for _ in range(2)]
    for b in buckets:
        b.load_weights(w)
        b.engine.set_mode('throughput')
    dev = buckets[0].engine.device
    host = []
    for i in range(2 * K):
        b = synth.make_inputs(d, seed=100 + i)
        if compact:
            b['image_feat_batch'], index = compact_rows(b['image_feat_batch'], half, Q)
            if index is not None:
                b['image_index_batch'] = index
        host.append({k: torch.as_tensor(np.ascontiguousarray(v)).pin_memory()
                     for k, v in b.items() if k in ('input_seq_batch', 'seq_length_batch', 'image_feat_batch',
                                                    'image_index_batch')})
    gt = torch.as_tensor(synth.template_layout_batch(d)).to(dev)
    for b in buckets:
        for k in range(K):
            b.slot(k)['gt_layout_batch'].copy_(gt)
    # compact feed: per slot a landing buffer in the container dtype and an index buffer (as DeviceFeeder keeps them)
    landing = [[{k: torch.empty(t.shape, dtype=t.dtype, device=dev) for k, t in host[s * K + k].items()
                 if k in ('image_feat_batch', 'image_index_batch')} for k in range(K)] for s in range(2)] if compact else None
    copy = torch.cuda.Stream(device=dev)
    comp = [torch.cuda.Stream(device=dev) for _ in buckets]
    copied = [torch.cuda.Event() for _ in buckets]
    released = [torch.cuda.Event() for _ in buckets]

    def one_pass(i, first):
        s = i & 1
        bk = buckets[s]
        with torch.cuda.stream(copy):
            if not first:
                copy.wait_event(released[s])
            for k in range(K):
                slot = bk.slot(k)
                for key, t in host[s * K + k].items():
                    (landing[s][k][key] if compact and key in landing[s][k] else slot[key]).copy_(t, non_blocking=True)
                if compact:
                    feed.expand(landing[s][k]['image_feat_batch'], landing[s][k].get('image_index_batch'),
                                slot['image_feat_batch'])
            copied[s].record(copy)
        with torch.cuda.stream(comp[s]):
            comp[s].wait_event(copied[s])
            bk.run(use_gt_layout=True)
            released[s].record(comp[s])

    for i in range(4):
        one_pass(i, i < 2)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(passes):
        one_pass(i, False)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    nq = passes * K * d.N
    feat_bytes = host[0]['image_feat_batch'].numel() * host[0]['image_feat_batch'].element_size()
    mb = passes * K * feat_bytes / 1e6
    if not compact:
        print('host-fed: %.1f questions/s, %.3f ms per batch of 64, H2D %.1f GB/s (features only)'
              % (nq / dt, 1e3 * dt / (passes * K), mb / 1e3 / dt))
        return
    print('host-fed (%s, %d question(s) per image): %.1f questions/s, %.3f ms per batch of 64, H2D %.1f GB/s '
          '(features only, %.2f MB per batch)' % (a.feat_dtype, Q, nq / dt, 1e3 * dt / (passes * K), mb / 1e3 / dt,
                                                  feat_bytes / 1e6))
    expand_alone(dev, half)


def vqa_run(a):
    """models_vqa, batch 128: the features of batch i+1 go host -> device -> slab (VQAEngine.fill_slab, on the copy
    stream) under the forward of batch i on the other slab"""
    import torch
    from n2nmn_amd import vqa, synth
    half, Q, passes = a.feat_dtype == 'float16', a.questions_per_image, a.passes
    d = vqa.VQADims(N=128)
    eng = vqa.VQAEngine(d)
    eng.load_weights(synth.make_weights_from_shapes(vqa.vqa_variable_shapes(d), seed=0))
    dev = eng.engine.device
    mix = (['_Find', '_Find', '_And', '_Describe'],) * 46 + (['_Find', '_Describe'],) * 43 + \
          (['_Find', '_Transform', '_Describe'],) * 9 + (['_Find', '_Transform', '_Find', '_And', '_Describe'],) * 2
    rng = np.random.default_rng(0)
    host, text, gts = [], [], []
    for i in range(2):
        lens = rng.integers(3, d.T_encoder + 1, size=d.N).astype(np.int32)
        seq = rng.integers(0, d.num_vocab_txt, size=(d.T_encoder, d.N)).astype(np.int32)
        seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
        feat = torch.relu(torch.randn((d.N, d.H, d.W, d.D), generator=torch.Generator().manual_seed(i))).numpy()
        rows, index = compact_rows(feat, half, Q)
        host.append((torch.as_tensor(rows).pin_memory(), index))
        text.append(dict(input_seq_batch=torch.as_tensor(seq).to(dev), seq_length_batch=torch.as_tensor(lens).to(dev)))
        order = rng.permutation(100)
        gts.append(np.ascontiguousarray(np.array(
            [eng.assembler.module_list2tokens(mix[order[n % 100]], d.T_decoder) for n in range(d.N)], np.int32).T))
    slabs = [eng.feature_slab(d.N) for _ in range(2)]
    copy, comp = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    copied = [torch.cuda.Event() for _ in slabs]
    released = [torch.cuda.Event() for _ in slabs]

    def one_pass(i, first):
        s = i & 1
        with torch.cuda.stream(copy):
            if not first:
                copy.wait_event(released[s])
            eng.fill_slab(slabs[s], host[s][0], host[s][1])
            copied[s].record(copy)
        with torch.cuda.stream(comp):
            comp.wait_event(copied[s])
            eng.forward(dict(text[s], image_feat_batch=slabs[s]), use_gt_layout=True, gt_layout=gts[s])
            released[s].record(comp)

    for i in range(4):
        one_pass(i, i < 2)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(passes):
        one_pass(i, False)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    feat_bytes = host[0][0].numel() * host[0][0].element_size()
    print('host-fed vqa (%s, %d question(s) per image): %.1f questions/s, %.3f ms per batch of 128, H2D %.1f GB/s '
          '(features only, %.1f MB per batch)' % (a.feat_dtype, Q, passes * d.N / dt, 1e3 * dt / passes,
                                                  passes * feat_bytes / 1e9 / dt, feat_bytes / 1e6))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--variant', choices=('clevr', 'vqa'), default='clevr')
    ap.add_argument('--feat-dtype', choices=('float32', 'float16'), default='float32')
    ap.add_argument('--questions-per-image', type=int, default=1, metavar='Q')
    ap.add_argument('--passes', type=int, default=40)
    ap.add_argument('--expand-only', action='store_true')
    a = ap.parse_args(argv)
    if a.questions_per_image < 1 or a.passes < 1:
        ap.error('--questions-per-image and --passes must be positive')
    if a.expand_only:
        import torch
        from n2nmn_amd import _lib
        _lib.lib()
        return expand_alone(torch.device('cuda', 0))
    (vqa_run if a.variant == 'vqa' else clevr)(a)


if __name__ == '__main__':
    main()
