"""VGG-16 pool5 features on the device: image -> the `image_feat` grid of the CLEVR entry points.

The reference stage is models_clevr/vgg_net.py::vgg_pool5 driven by
exp_clevr/data/extract_visual_features_vgg_pool5.py: a 320 x 480 RGB image minus `channel_mean`, 13 SAME
3x3 convolutions with bias and ReLU, five 2x2 max-pools, a (1, 10, 15, 512) float32 grid saved per image.
Here it is `VGGPool5` over the n2nmn_vgg handle of include/n2nmn.h section 9 (HIP kernels, exact fp32):

    vgg = VGGPool5(max_N=8)                     # 320 x 480 unless max_H / max_W say otherwise
    vgg.load_checkpoint('vgg_net.tfmodel')      # variables vgg_net/convX_Y/{weights,biases}
    feat = vgg.forward(images)                  # uint8 or float32 [N, H, W, 3] -> device [N, H/32, W/32, 512]
    engine.forward({'image_feat_batch': feat, ...})      # no trip through the host

    python -m n2nmn_amd.vgg_net --weights vgg_net.tfmodel --images DIR --out DIR

The published checkpoint (the reference's exp_clevr/tfmodel/vgg_net/download_vgg_net.sh fetches it) is 59 MB
and is NOT part of this repository, nor was it available where this code was written: the tests and the
fixture run on `synthetic_weights`, and no run with the real weights has been made.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import Dict, List, Tuple

import numpy as np

from . import _lib, feed

channel_mean = np.array([123.68, 116.779, 103.939], dtype=np.float32)      # vgg_net.py:14

_WIDTHS = ((1, 2, 64), (2, 2, 128), (3, 3, 256), (4, 3, 512), (5, 3, 512))
CONV_LAYERS: Tuple[str, ...] = tuple('conv%d_%d' % (g, j + 1) for g, n, _ in _WIDTHS for j in range(n))
LAYERS: Tuple[str, ...] = tuple(
    name for g, n, _ in _WIDTHS for name in ['conv%d_%d' % (g, j + 1) for j in range(n)] + ['pool%d' % g])


def variable_shapes() -> List[Tuple[str, Tuple[int, ...]]]:
    """The 26 variables of vgg_pool5 in creation order, by their names inside the scope:
    convX_Y/weights [3, 3, Cin, Cout] (HWIO), convX_Y/biases [Cout]."""
    out, cin = [], 3
    for g, n, cout in _WIDTHS:
        for j in range(n):
            out.append(('conv%d_%d/weights' % (g, j + 1), (3, 3, cin, cout)))
            out.append(('conv%d_%d/biases' % (g, j + 1), (cout,)))
            cin = cout
    return out


def synthetic_weights(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded stand-in for the 59 MB checkpoint: all 26 variables as float32, drawn from ONE
    np.random.RandomState(seed) in the order of `variable_shapes()` -- for each layer conv1_1 ... conv5_3 first
    the weights, `randn(3, 3, Cin, Cout) * sqrt(2 / (9 Cin))` (He scaling: activations keep their scale through
    the 13 ReLU layers), then the biases, `randn(Cout) * 0.1`.  The fixture generator
    (tests/golden/make_vgg_golden.py) and the tests use exactly this."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in variable_shapes():
        if name.endswith('weights'):
            out[name] = (rs.randn(*shape) * np.sqrt(2.0 / (9 * shape[2]))).astype(np.float32)
        else:
            out[name] = (rs.randn(*shape) * 0.1).astype(np.float32)
    return out


def read_checkpoint_weights(path: str, scope: str = 'vgg_net') -> Dict[str, np.ndarray]:
    """The 26 variables of a TF-V2 checkpoint prefix holding `<scope>/convX_Y/{weights,biases}` -- what the
    reference's `tf.train.Saver().restore(sess, vgg_net_model)` reads for `vgg_pool5(image_batch, 'vgg_net')` --
    keyed by their names inside the scope, shapes checked."""
    from . import tf_checkpoint
    shapes = variable_shapes()
    got = tf_checkpoint.read_checkpoint(path, names=['%s/%s' % (scope, n) for n, _ in shapes])
    out = {}
    for n, shape in shapes:
        a = got['%s/%s' % (scope, n)]
        if tuple(a.shape) != shape:
            raise ValueError('vgg_net: %s/%s has shape %s in %s, expected %s' % (scope, n, tuple(a.shape), path, shape))
        out[n] = np.ascontiguousarray(a, np.float32)
    return out


def pool5_shape(N: int, H: int, W: int) -> Tuple[int, int, int, int]:
    for _ in range(5):
        H, W = (H + 1) // 2, (W + 1) // 2
    return (N, H, W, 512)


class VGGPool5:
    """vgg_pool5 on one device.  Buffers for up to max_N images of max_H x max_W are allocated here, once."""

    def __init__(self, max_N: int = 1, max_H: int = 320, max_W: int = 480, device: int = 0):
        import torch
        self._lib = _lib.lib()
        self.device = torch.device('cuda', device)
        self.max_N, self.max_H, self.max_W = int(max_N), int(max_H), int(max_W)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.n2nmn_vgg_create(device, self.max_N, self.max_H, self.max_W, C.byref(h)))
        self._h = h
        self._loaded = False

    def close(self):
        if getattr(self, '_h', None):
            self._lib.n2nmn_vgg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- weights --------------------------------------------------------------------------------
    def load_weights(self, mapping):
        """mapping: 'convX_Y/weights' / 'convX_Y/biases' -> array, all 26 (a missing one is a KeyError).  Extra
        keys are an error too: a misspelt name must not pass silently."""
        import torch
        names = [n for n, _ in variable_shapes()]
        extra = sorted(set(mapping) - set(names))
        if extra:
            raise KeyError('vgg_net: unknown variables %s' % extra)
        for name in names:
            if name not in mapping:
                raise KeyError('vgg_net: variable %r is missing' % name)
            t = torch.as_tensor(np.asarray(mapping[name])).to(device=self.device, dtype=torch.float32).contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            _lib.check(self._lib.n2nmn_vgg_set_weight(self._h, name.encode(), t.data_ptr(), shape, t.dim()))
        _lib.check(self._lib.n2nmn_vgg_commit(self._h, self.stream()))
        self._loaded = True

    def load_checkpoint(self, path: str, scope: str = 'vgg_net'):
        """load_weights(read_checkpoint_weights(path, scope))"""
        self.load_weights(read_checkpoint_weights(path, scope))

    # ---- forward --------------------------------------------------------------------------------
    def _images(self, images):
        import torch
        t = torch.as_tensor(images) if not isinstance(images, torch.Tensor) else images
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError('vgg_net: images must be [N, H, W, 3] RGB, got %s' % (tuple(t.shape),))
        if t.dtype != torch.uint8:
            t = t.to(torch.float32)
        return t.to(self.device).contiguous()

    def forward(self, images, out_dtype=None):
        """images: uint8 or float [N, H, W, 3] RAW RGB values (host or device; channel_mean is subtracted by the
        first kernel) -> float32 DEVICE tensor [N, ceil(H/32), ceil(W/32), 512] on the current stream.  Nothing is
        copied to the host: hand the result to Engine / NMN3Model / the super-bucket feeder as image_feat.
        out_dtype='float16': the grid narrowed to IEEE half on the device (n2nmn_features_narrow, round to nearest
        even): half the D2H copy and half the file of an extraction run; Engine takes it as it is."""
        import torch
        if not self._loaded:
            raise RuntimeError('vgg_net: no weights loaded (load_weights / load_checkpoint)')
        t = self._images(images)
        N, H, W, _ = t.shape
        out = torch.empty(pool5_shape(N, H, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.n2nmn_vgg_forward(self._h, t.data_ptr(), 1 if t.dtype == torch.uint8 else 0,
                                                   N, H, W, out.data_ptr(), self.stream()))
        return feed.narrow(out) if feed.half_requested(out_dtype) else out

    def layer(self, name: str):
        """Dense device copy [N, h, w, C] of one layer's activation (after ReLU) of the last forward."""
        import torch
        shape = (C.c_int64 * 4)()
        _lib.check(self._lib.n2nmn_vgg_get_layer(self._h, name.encode(), None, 0, shape, self.stream()))
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.n2nmn_vgg_get_layer(self._h, name.encode(), out.data_ptr(), out.numel(), shape,
                                                 self.stream()))
        return out

    def replay_us(self, name: str, iters: int = 20) -> float:
        """mean microseconds of one launch of layer `name` of the last forward (n2nmn_vgg_debug_replay)"""
        us = C.c_double()
        _lib.check(self._lib.n2nmn_vgg_debug_replay(self._h, name.encode(), iters, C.byref(us), self.stream()))
        return us.value


def _dev32(x, device):
    import torch
    return torch.as_tensor(x).to(device=device, dtype=torch.float32).contiguous()


def conv3x3_relu(x, w, b, device: int = 0):
    """One SAME 3x3 conv + bias + ReLU on dense tensors through the forward's kernel (n2nmn_vgg_debug_conv)."""
    import torch
    dev = torch.device('cuda', device)
    x, w, b = _dev32(x, dev), _dev32(w, dev), _dev32(b, dev)
    N, H, W, Cin = x.shape
    Cout = w.shape[3]
    if tuple(w.shape) != (3, 3, Cin, Cout) or tuple(b.shape) != (Cout,):
        raise ValueError('vgg_net.conv3x3_relu: weights %s / biases %s do not fit input %s'
                         % (tuple(w.shape), tuple(b.shape), tuple(x.shape)))
    out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().n2nmn_vgg_debug_conv(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), N, H, W,
                                               Cin, Cout, torch.cuda.current_stream(dev).cuda_stream))
    return out


def max_pool_2x2(x, device: int = 0):
    """One 2x2 stride-2 SAME max-pool on a dense tensor through the forward's kernel (n2nmn_vgg_debug_pool)."""
    import torch
    dev = torch.device('cuda', device)
    x = _dev32(x, dev)
    N, H, W, Cc = x.shape
    out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, Cc), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().n2nmn_vgg_debug_pool(x.data_ptr(), out.data_ptr(), N, H, W, Cc,
                                               torch.cuda.current_stream(dev).cuda_stream))
    return out


# ---- dataset extraction (extract_visual_features_vgg_pool5.py:40-57) -------------------------------
def _read_rgb(path: str) -> np.ndarray:
    """what `skimage.io.imread(impath)[..., :3]` yields for the PNGs of CLEVR: uint8 [H, W, 3], alpha dropped"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ('RGB', 'RGBA'):
            im = im.convert('RGB')
        a = np.asarray(im)
    return np.ascontiguousarray(a[..., :3])


def extract_dataset_pool5(image_dir: str, save_dir: str, ext_filter: str = '*.png', vgg: VGGPool5 = None,
                          batch_size: int = 8, verbose: bool = False, dtype=None) -> int:
    """The reference script's contract: for every image matching `ext_filter` in `image_dir`, one
    `<image name>.npy` in `save_dir` holding pool5 as float32 (1, H/32, W/32, 512); files that exist are skipped.
    dtype='float16': float16 files of the same shape, narrowed on the device (DataReader's feature_dtype='float16'
    loads them as they are).
    Consecutive images of equal size run as one batch of up to `batch_size` (the handle's max_N).  Returns the
    number of files written.  vgg: a loaded VGGPool5 (its max_N / max_H / max_W bound what can be read)."""
    if vgg is None:
        raise ValueError('extract_dataset_pool5: pass a VGGPool5 with its weights loaded')
    os.makedirs(save_dir, exist_ok=True)
    todo = []
    for impath in sorted(glob.glob(image_dir + '/' + ext_filter)):
        image_name = os.path.basename(impath).split('.')[0]
        save_path = os.path.join(save_dir, image_name + '.npy')
        if not os.path.exists(save_path):
            todo.append((impath, save_path))
    batch_size = max(1, min(batch_size, vgg.max_N))
    written = 0
    pending: List[Tuple[str, np.ndarray]] = []

    def flush():
        nonlocal written
        if not pending:
            return
        feat = vgg.forward(np.stack([im for _, im in pending]), out_dtype=dtype).cpu().numpy()
        for i, (save_path, _) in enumerate(pending):
            np.save(save_path, feat[i:i + 1])
            written += 1
        if verbose:
            print('processed %d / %d' % (written, len(todo)))
        pending.clear()

    for impath, save_path in todo:
        im = _read_rgb(impath)
        if pending and (pending[0][1].shape != im.shape or len(pending) == batch_size):
            flush()
        pending.append((save_path, im))
    flush()
    return written


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='VGG-16 pool5 features of every image of a directory, one .npy each')
    ap.add_argument('--weights', required=True, help='TF checkpoint prefix holding vgg_net/convX_Y/{weights,biases}')
    ap.add_argument('--images', required=True, help='directory of images')
    ap.add_argument('--out', required=True, help='directory the .npy files go to')
    ap.add_argument('--ext', default='*.png')
    ap.add_argument('--scope', default='vgg_net')
    ap.add_argument('--height', type=int, default=320)
    ap.add_argument('--width', type=int, default=480)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--dtype', choices=('float32', 'float16'), default='float32', help='container of the .npy files')
    a = ap.parse_args(argv)
    vgg = VGGPool5(max_N=a.batch, max_H=a.height, max_W=a.width, device=a.device)
    vgg.load_checkpoint(a.weights, scope=a.scope)
    n = extract_dataset_pool5(a.images, a.out, a.ext, vgg=vgg, batch_size=a.batch, verbose=True, dtype=a.dtype)
    print('wrote %d files to %s' % (n, a.out))


if __name__ == '__main__':
    main()
