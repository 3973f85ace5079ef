#!/usr/bin/env python3
"""Generate tests/golden/vgg_golden.npz by RUNNING THE REFERENCE'S OWN models_clevr/vgg_net.py.

oracle/tf1_stub executes every tf op eagerly on torch CPU tensors in float64, so the UNMODIFIED
`vgg_net.vgg_pool5` (and util/cnn.py's conv_relu_layer / pooling_layer under it) computes the numbers of this
fixture from preloaded weights -- `n2nmn_amd.vgg_net.synthetic_weights(seed)`, because the published 59 MB
checkpoint is neither a possible fixture nor available here -- and from `im - vgg_net.channel_mean` exactly
as exp_clevr/data/extract_visual_features_vgg_pool5.py:36 forms it.

The fixture holds only data: the seed, the uint8 images, the fp64 pool5 outputs, and the names and shapes of
the variables the reference code asked the stub for.  Two cases, the smallest that reach every way the kernels
can go wrong:
  A: N = 2, 34 x 50   every pool sees an odd extent (34 17 9 5 3 2 / 50 25 13 7 4 2), N H W = 3400 is no
                      multiple of the 128-row tile, tiles straddle row ends and the boundary of the two images
  B: N = 1, 64 x 96   even at every level, like 320 x 480; a 2 x 3 grid

Only works where the reference checkout is present.  No bytecode is written into the reference tree.
Usage:  python tests/golden/make_vgg_golden.py [--check]
(--check regenerates in memory and compares with the committed file instead of writing it).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
OUT = os.path.join(HERE, 'vgg_golden.npz')
SEED = 0
CASES = (('A', 2, 34, 50, 1000), ('B', 1, 64, 96, 1001))      # name, N, H, W, image seed


def setup_reference_imports():
    """stub tensorflow first on sys.path, then the reference checkout, then this repo."""
    for p in (ROOT, REF, os.path.join(ROOT, 'oracle', 'tf1_stub')):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    import tensorflow as tf
    assert 'tf1_stub' in tf.__file__
    return tf


def images(N, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)


def generate():
    tf = setup_reference_imports()
    import torch
    from models_clevr import vgg_net                      # the reference's, unmodified
    from n2nmn_amd import vgg_net as ours
    assert vgg_net.__file__.startswith(REF)
    weights = ours.synthetic_weights(SEED)
    out = {'seed': np.int64(SEED)}
    for name, N, H, W, iseed in CASES:
        tf.reset_default_graph()
        tf.config.float_dtype = torch.float64
        tf.config.preloaded = {'vgg_net/' + k: np.asarray(v, np.float64) for k, v in weights.items()}
        tf.config.strict_preload = True
        im = images(N, H, W, iseed)
        im_val = im - vgg_net.channel_mean               # extract_visual_features_vgg_pool5.py:36
        pool5 = vgg_net.vgg_pool5(torch.as_tensor(im_val.astype(np.float64)), 'vgg_net')
        out['images_' + name] = im
        out['pool5_' + name] = pool5.detach().numpy().astype(np.float64)
        asked = [[k[len('vgg_net/'):], list(v.shape)] for k, v in tf._variables.items() if k.startswith('vgg_net/')]
    out['variables'] = np.array(json.dumps(asked))
    return out


def main():
    new = generate()
    if '--check' in sys.argv:
        old = np.load(OUT)
        worst = 0.0
        assert sorted(old.files) == sorted(new), (sorted(old.files), sorted(new))
        for k in sorted(new):
            a, b = np.asarray(old[k]), np.asarray(new[k])
            if a.dtype.kind in 'US':
                assert str(a) == str(b), k
                continue
            assert a.shape == b.shape and a.dtype == b.dtype, k
            worst = max(worst, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
        print('vgg_golden.npz: max abs difference %g' % worst)
        sys.exit(0 if worst == 0.0 else 1)
    np.savez_compressed(OUT, **new)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    for k in sorted(new):
        print(' ', k, np.asarray(new[k]).shape, np.asarray(new[k]).dtype)


if __name__ == '__main__':
    main()
