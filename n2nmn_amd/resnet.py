"""ResNet-152 res5c features on the device: image -> the (14, 14, 2048) `image_feat` grid of the VQA entry points.

The reference does not compute these features.  Its README asks for "the res5c layer of the ResNet-152 network ...
shape (1, 14, 14, 2048) ... HxWxC", sends the reader to an outside Caffe installation for them, and
exp_vqa/data/build_vqa*_imdb.py only points at `./resnet_res5c/<set>/<image name>.npy`.  The network here is
therefore He et al.'s ResNet-152 as deployed in Caffe, restated from its PUBLISHED description -- no file of the
reference or of this repository's surroundings defines it:

    conv1  7x7 / 2, pad 3, 3 -> 64, batch-norm, scale, ReLU
    pool1  max 3x3 / 2, pad 0, Caffe ceil mode (extent ceil((n - 3) / 2) + 1, overhanging windows clipped)
    res2 .. res5: (3, 8, 36, 3) bottleneck blocks of width (64, 128, 256, 512), 4 x expansion;
      branch2a 1x1 + BN + ReLU, branch2b 3x3 pad 1 + BN + ReLU, branch2c 1x1 + BN, out = relu(branch2c + shortcut);
      the first block of a stage has the projection shortcut branch1 (1x1 + BN), and in res3, res4, res5 it has
      stride 2 on branch2a AND branch1 (every 3x3 is stride 1)
    batch-norm in inference form, eps 1e-5, followed by Caffe's scale layer (gamma, beta)

Here it is `ResNetRes5c` over the n2nmn_resnet handle of include/n2nmn.h section 10 (HIP kernels, exact fp32):

    net = ResNetRes5c(max_N=8)                  # 448 x 448 unless max_H / max_W say otherwise
    net.load_weights(load_npz('resnet152.npz')) # raw Caffe-named arrays, or already folded ones
    feat = net.forward(images)                  # uint8 or float32 [N, H, W, 3] -> device [N, H/32, W/32, 2048]
    vqa_engine.forward({'image_feat_batch': feat, ...})      # no trip through the host

    python -m n2nmn_amd.resnet --weights resnet152.npz --images DIR --out resnet_res5c/train2014

Batch-norm and scale are folded into the convolutions on the host, in fp64 (`fold_batchnorm`), so the device
runs convolution + bias (+ residual) (+ ReLU) only.

NOT verified, and not verifiable where this code was written: the published weights (a 230 MB .caffemodel) were
not available, and neither Caffe nor its protobuf schema, so there is NO .caffemodel reader here -- export the
blobs to an .npz under the names `fold_batchnorm` documents (`load_npz`).  The tests run on
`synthetic_weights` against tests/resnet_oracle.py, a torch restatement of the description above; no run with
the real weights has been made, and the channel order / mean the published weights expect (they were trained on
BGR images, see `load_npz(bgr_conv1=True)`) and the image resizing of the original feature extraction are
the caller's to match.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _lib, feed
from .vgg_net import channel_mean, _read_rgb

BLOCKS_152: Tuple[int, int, int, int] = (3, 8, 36, 3)
BN_EPS = 1e-5


def block_names(blocks: Sequence[int] = BLOCKS_152) -> List[str]:
    """Caffe's block names: a stage of up to 3 blocks is lettered (res2a res2b res2c), a longer one is
    a, b1, b2, ... (res4a res4b1 ... res4b35) -- the naming of the published ResNet-101 / -152 definitions."""
    out = []
    for st, n in enumerate(blocks):
        for j in range(n):
            out.append('res%d%s' % (st + 2, 'abc'[j] if (n <= 3 or j == 0) else 'b%d' % j))
    return out


def _layers(blocks: Sequence[int], base_width: int) -> List[Tuple[str, Tuple[int, int, int, int]]]:
    """(convolution name, HWIO weight shape) in execution order"""
    if len(blocks) != 4 or min(blocks) < 1:
        raise ValueError('resnet: blocks must be four positive counts, got %r' % (tuple(blocks),))
    out = [('conv1', (7, 7, 3, base_width))]
    names = iter(block_names(blocks))
    cin = base_width
    for st, n in enumerate(blocks):
        width = base_width << st
        for j in range(n):
            b = next(names)
            if j == 0:
                out.append((b + '_branch1', (1, 1, cin, 4 * width)))
            out.append((b + '_branch2a', (1, 1, cin, width)))
            out.append((b + '_branch2b', (3, 3, width, width)))
            out.append((b + '_branch2c', (1, 1, width, 4 * width)))
            cin = 4 * width
    return out


def layer_names(blocks: Sequence[int] = BLOCKS_152) -> List[str]:
    """The convolutions in execution order: conv1, res2a_branch1, res2a_branch2a, ... (155 for ResNet-152).
    `ResNetRes5c.layer` also knows 'pool1'; '<block>_branch2c' yields the BLOCK output (see include/n2nmn.h)."""
    return [n for n, _ in _layers(blocks, 64)]


def variable_shapes(blocks: Sequence[int] = BLOCKS_152, base_width: int = 64) -> List[Tuple[str, Tuple[int, ...]]]:
    """The FOLDED variables the device holds, in execution order: <layer>/weights [k, k, Cin, Cout] (HWIO),
    <layer>/biases [Cout]."""
    out = []
    for name, shape in _layers(blocks, base_width):
        out.append((name + '/weights', shape))
        out.append((name + '/biases', (shape[3],)))
    return out


def pool_extent(n: int) -> int:
    """pool1's output extent, Caffe ceil mode: ceil((n - 3) / 2) + 1"""
    return max(-((n - 3) // -2), 0) + 1


def res5c_shape(N: int, H: int, W: int, base_width: int = 64) -> Tuple[int, int, int, int]:
    def ext(n):
        n = (n - 1) // 2 + 1               # conv1
        n = pool_extent(n)                 # pool1
        for _ in range(3):                 # res3a, res4a, res5a
            n = (n - 1) // 2 + 1
        return n
    return (N, ext(H), ext(W), 32 * base_width)


def bn_names(conv: str) -> Tuple[str, str]:
    """Caffe's batch-norm and scale layer of a convolution: conv1 -> bn_conv1, scale_conv1;
    res2a_branch2a -> bn2a_branch2a, scale2a_branch2a"""
    tail = '_conv1' if conv == 'conv1' else conv[3:]
    return 'bn' + tail, 'scale' + tail


def fold_batchnorm(raw: Dict[str, np.ndarray], eps: float = BN_EPS) -> Dict[str, np.ndarray]:
    """Raw Caffe-named arrays -> the folded pair per convolution, computed in fp64, stored as float32.

    Per convolution <conv> (bn, scale = bn_names(<conv>)) `raw` holds
        <conv>/weights [k, k, Cin, Cout] (HWIO; Caffe's OIHW blob transposed (2, 3, 1, 0)),  <conv>/biases [Cout] optional,
        <bn>/mean, <bn>/variance [Cout] (Caffe's blobs 0 and 1 DIVIDED by its blob 2, the moving-average factor),
        <scale>/gamma, <scale>/beta [Cout]
    and the result holds, with s = gamma / sqrt(variance + eps),
        <conv>/weights = W * s (per output channel),   <conv>/biases = beta - mean * s (+ bias * s)."""
    out = {}
    convs = [k[:-len('/weights')] for k in raw if k.endswith('/weights')]
    for conv in convs:
        bn, sc = bn_names(conv)
        w = np.asarray(raw[conv + '/weights'], np.float64)
        s = np.asarray(raw[sc + '/gamma'], np.float64) / np.sqrt(np.asarray(raw[bn + '/variance'], np.float64) + eps)
        b = np.asarray(raw[sc + '/beta'], np.float64) - np.asarray(raw[bn + '/mean'], np.float64) * s
        if conv + '/biases' in raw:
            b = b + np.asarray(raw[conv + '/biases'], np.float64) * s
        out[conv + '/weights'] = (w * s).astype(np.float32)
        out[conv + '/biases'] = b.astype(np.float32)
    return out


def synthetic_weights(seed: int = 0, blocks: Sequence[int] = BLOCKS_152, base_width: int = 64) -> Dict[str, np.ndarray]:
    """Seeded stand-in for the published weights, in RAW form (fold_batchnorm's input), float32, drawn from ONE
    np.random.RandomState(seed).  For each convolution in `layer_names` order, five draws in this order:
        weights   randn(k, k, Cin, Cout) * sqrt(2 / (k k Cin))      (He scaling)
        mean      randn(Cout) * 0.1
        variance  0.9 + 0.2 * rand(Cout)
        gamma     1 + 0.1 * randn(Cout);  times 0.25 for a block's last layer, branch2c
        beta      randn(Cout) * 0.1
    Statistics near identity keep the activations' scale through the depth; the small gamma of branch2c keeps the
    residual sum from growing over 50 blocks (each block adds about 1/16 of its input's variance)."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in _layers(blocks, base_width):
        k, _, cin, cout = shape
        bn, sc = bn_names(name)
        out[name + '/weights'] = (rs.randn(*shape) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
        out[bn + '/mean'] = (rs.randn(cout) * 0.1).astype(np.float32)
        out[bn + '/variance'] = (0.9 + 0.2 * rs.rand(cout)).astype(np.float32)
        g = 1.0 + 0.1 * rs.randn(cout)
        out[sc + '/gamma'] = (g * (0.25 if name.endswith('_branch2c') else 1.0)).astype(np.float32)
        out[sc + '/beta'] = (rs.randn(cout) * 0.1).astype(np.float32)
    return out


def is_raw(mapping) -> bool:
    return any(k.startswith('bn') for k in mapping)


def load_npz(path: str, bgr_conv1: bool = False) -> Dict[str, np.ndarray]:
    """An .npz keyed by the names of `fold_batchnorm` (raw: folded here) or of `variable_shapes` (already folded:
    taken as it is) -> the folded mapping `ResNetRes5c.load_weights` takes.  bgr_conv1: the weights were trained
    on BGR images (the published ones were); conv1's input-channel axis is reversed so that RGB images can be
    fed -- reverse `channel_mean` to match.  A .caffemodel is NOT read: no Caffe, no protobuf schema here."""
    with np.load(path) as z:
        m = {k: z[k] for k in z.files}
    m = fold_batchnorm(m) if is_raw(m) else {k: np.asarray(v, np.float32) for k, v in m.items()}
    if bgr_conv1:
        m['conv1/weights'] = np.ascontiguousarray(m['conv1/weights'][:, :, ::-1, :])
    return m


class ResNetRes5c:
    """The network up to its last block on one device.  Buffers for up to max_N images of max_H x max_W are
    allocated here, once.  blocks / base_width other than (3, 8, 36, 3) / 64 give shallow or narrow nets for
    tests; base_width must be a multiple of 32."""

    def __init__(self, max_N: int = 1, max_H: int = 448, max_W: int = 448, blocks: Sequence[int] = BLOCKS_152,
                 base_width: int = 64, channel_mean=channel_mean, device: int = 0):
        import torch
        self._lib = _lib.lib()
        self.device = torch.device('cuda', device)
        self.max_N, self.max_H, self.max_W = int(max_N), int(max_H), int(max_W)
        self.blocks, self.base_width = tuple(int(b) for b in blocks), int(base_width)
        if len(self.blocks) != 4:
            raise ValueError('resnet: blocks must be four counts, got %r' % (self.blocks,))
        mean = np.asarray(channel_mean, np.float32).reshape(3)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.n2nmn_resnet_create(device, self.max_N, self.max_H, self.max_W,
                                                     (C.c_int * 4)(*self.blocks), self.base_width, C.byref(h)))
        self._h = h
        _lib.check(self._lib.n2nmn_resnet_set_mean(self._h, (C.c_float * 3)(*mean.tolist())))
        self._loaded = False

    def close(self):
        if getattr(self, '_h', None):
            self._lib.n2nmn_resnet_destroy(self._h)
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
        """mapping: raw (fold_batchnorm's input; folded here) or folded ('<layer>/weights', '<layer>/biases' for
        every layer of `variable_shapes`).  A missing or an extra key is a KeyError."""
        import torch
        if is_raw(mapping):
            mapping = fold_batchnorm(mapping)
        names = [n for n, _ in variable_shapes(self.blocks, self.base_width)]
        extra = sorted(set(mapping) - set(names))
        if extra:
            raise KeyError('resnet: unknown variables %s' % extra[:4])
        self._loaded = False
        for name in names:
            if name not in mapping:
                raise KeyError('resnet: variable %r is missing' % name)
            t = torch.as_tensor(np.asarray(mapping[name])).to(device=self.device, dtype=torch.float32).contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            _lib.check(self._lib.n2nmn_resnet_set_weight(self._h, name.encode(), t.data_ptr(), shape, t.dim()))
        _lib.check(self._lib.n2nmn_resnet_commit(self._h, self.stream()))
        self._loaded = True

    # ---- forward --------------------------------------------------------------------------------
    def _images(self, images):
        import torch
        t = torch.as_tensor(images) if not isinstance(images, torch.Tensor) else images
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError('resnet: images must be [N, H, W, 3], got %s' % (tuple(t.shape),))
        if t.dtype != torch.uint8:
            t = t.to(torch.float32)
        return t.to(self.device).contiguous()

    def forward(self, images, out_dtype=None):
        """images: uint8 or float [N, H, W, 3] RAW pixel values (host or device; the channel mean is subtracted by
        the first kernel) -> float32 DEVICE tensor [N, h, w, 32 base_width] on the current stream (448 x 448 ->
        14 x 14 x 2048).  Nothing is copied to the host: hand the result to VQAEngine.forward as image_feat_batch.
        Before load_weights the library refuses (N2NMN_ENOWEIGHT).  out_dtype='float16': the grid narrowed to IEEE
        half on the device (n2nmn_features_narrow, round to nearest even)."""
        import torch
        t = self._images(images)
        N, H, W, _ = t.shape
        out = torch.empty(res5c_shape(N, H, W, self.base_width), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.n2nmn_resnet_forward(self._h, t.data_ptr(), 1 if t.dtype == torch.uint8 else 0,
                                                      N, H, W, out.data_ptr(), self.stream()))
        return feed.narrow(out) if feed.half_requested(out_dtype) else out

    def layer(self, name: str):
        """Dense device copy [N, h, w, C] of one layer's output for the last forward's images: 'conv1', 'pool1',
        any name of `layer_names`; '<block>_branch2c' (or '<block>') is the block output after the sum and ReLU."""
        import torch
        shape = (C.c_int64 * 4)()
        _lib.check(self._lib.n2nmn_resnet_get_layer(self._h, name.encode(), None, 0, shape, self.stream()))
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.n2nmn_resnet_get_layer(self._h, name.encode(), out.data_ptr(), out.numel(), shape,
                                                    self.stream()))
        return out

    def replay_us(self, name: str = '', iters: int = 20) -> float:
        """mean microseconds of one launch of layer `name` of the last forward, or of the whole network for ''
        (n2nmn_resnet_debug_replay)"""
        us = C.c_double()
        _lib.check(self._lib.n2nmn_resnet_debug_replay(self._h, name.encode(), iters, C.byref(us), self.stream()))
        return us.value


# ---- single operations through the forward's kernels (tests) ------------------------------------------
def _dev32(x, dev):
    import torch
    return torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()


def stem_conv(images, w, b, mean=channel_mean, device: int = 0):
    """relu(conv7x7 stride 2 pad 3 (images - mean) + b): images [N, H, W, 3] uint8 or float, w [7, 7, 3, Cout]"""
    import torch
    dev = torch.device('cuda', device)
    t = torch.as_tensor(images)
    t = (t if t.dtype == torch.uint8 else t.to(torch.float32)).to(dev).contiguous()
    w, b = _dev32(w, dev), _dev32(b, dev)
    N, H, W, _ = t.shape
    Cout = w.shape[3]
    if tuple(w.shape) != (7, 7, 3, Cout) or tuple(b.shape) != (Cout,) or t.shape[3] != 3:
        raise ValueError('resnet.stem_conv: weights %s / biases %s / images %s' % (tuple(w.shape), tuple(b.shape), tuple(t.shape)))
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout), dtype=torch.float32, device=dev)
    m = (C.c_float * 3)(*np.asarray(mean, np.float32).reshape(3).tolist())
    _lib.check(_lib.lib().n2nmn_resnet_debug_stem(t.data_ptr(), 1 if t.dtype == torch.uint8 else 0, w.data_ptr(),
                                                  b.data_ptr(), m, out.data_ptr(), N, H, W, Cout,
                                                  torch.cuda.current_stream(dev).cuda_stream))
    return out


def max_pool_3x3_s2(x, device: int = 0):
    """pool1 on a dense [N, H, W, C] tensor"""
    import torch
    dev = torch.device('cuda', device)
    x = _dev32(x, dev)
    N, H, W, Cc = x.shape
    out = torch.empty((N, pool_extent(H), pool_extent(W), Cc), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().n2nmn_resnet_debug_pool(x.data_ptr(), out.data_ptr(), N, H, W, Cc,
                                                  torch.cuda.current_stream(dev).cuda_stream))
    return out


def conv1x1(x, w, b, stride: int = 1, residual=None, relu: bool = True, device: int = 0):
    """act(conv1x1 stride s (x) + b (+ residual)): x [N, H, W, Cin], w [Cin, Cout] or [1, 1, Cin, Cout],
    residual [N, ho, wo, Cout] or None"""
    import torch
    dev = torch.device('cuda', device)
    x, w, b = _dev32(x, dev), _dev32(w, dev), _dev32(b, dev)
    N, H, W, Cin = x.shape
    w = w.reshape(-1, w.shape[-1])
    Cout = w.shape[1]
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = None if residual is None else _dev32(residual, dev)
    if w.shape[0] != Cin or tuple(b.shape) != (Cout,) or (r is not None and tuple(r.shape) != (N, ho, wo, Cout)):
        raise ValueError('resnet.conv1x1: operands do not fit input %s' % (tuple(x.shape),))
    out = torch.empty((N, ho, wo, Cout), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().n2nmn_resnet_debug_conv1x1(x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                     None if r is None else r.data_ptr(), out.data_ptr(), N, H, W,
                                                     Cin, Cout, stride, 1 if relu else 0,
                                                     torch.cuda.current_stream(dev).cuda_stream))
    return out


# ---- dataset extraction: the resnet_res5c/<set>/ directory of exp_vqa/data/build_vqa*_imdb.py -------------
def _read_resized(path: str, size: int) -> np.ndarray:
    """uint8 [size, size, 3] RGB; bilinear (PIL).  What the original extraction resized with is not recorded in
    the reference; 448 x 448 is what its (14, 14, 2048) grid implies."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert('RGB')
        if size and im.size != (size, size):
            im = im.resize((size, size), Image.BILINEAR)
        return np.ascontiguousarray(np.asarray(im)[..., :3])


def extract_dataset_res5c(image_dir: str, save_dir: str, ext_filter: str = '*.jpg', net: ResNetRes5c = None,
                          size: int = 448, batch_size: int = 8, verbose: bool = False, dtype=None) -> int:
    """For every image matching `ext_filter` in `image_dir`, one `<image name>.npy` in `save_dir` holding the
    features as float32 (1, size/32, size/32, 2048) -- the `feature_path` build_vqa_imdb.py:53 records; files that
    exist are skipped.  size = 0 keeps each image's own extent.  dtype='float16': float16 files of the same shape,
    narrowed on the device.  Returns the number of files written."""
    if net is None:
        raise ValueError('extract_dataset_res5c: pass a ResNetRes5c with its weights loaded')
    os.makedirs(save_dir, exist_ok=True)
    todo = []
    for impath in sorted(glob.glob(image_dir + '/' + ext_filter)):
        save_path = os.path.join(save_dir, os.path.basename(impath).split('.')[0] + '.npy')
        if not os.path.exists(save_path):
            todo.append((impath, save_path))
    batch_size = max(1, min(batch_size, net.max_N))
    written = 0
    pending: List[Tuple[str, np.ndarray]] = []

    def flush():
        nonlocal written
        if not pending:
            return
        feat = net.forward(np.stack([im for _, im in pending]), out_dtype=dtype).cpu().numpy()
        for i, (save_path, _) in enumerate(pending):
            np.save(save_path, feat[i:i + 1])
            written += 1
        if verbose:
            print('processed %d / %d' % (written, len(todo)))
        pending.clear()

    for impath, save_path in todo:
        im = _read_resized(impath, size) if size else _read_rgb(impath)
        if pending and (pending[0][1].shape != im.shape or len(pending) == batch_size):
            flush()
        pending.append((save_path, im))
    flush()
    return written


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='ResNet-152 res5c features of every image of a directory, one .npy each')
    ap.add_argument('--weights', required=True, help='.npz of raw (Caffe-named) or folded arrays, see load_npz')
    ap.add_argument('--images', required=True, help='directory of images')
    ap.add_argument('--out', required=True, help='directory the .npy files go to (resnet_res5c/<set>)')
    ap.add_argument('--size', type=int, default=448, help='images are resized to size x size')
    ap.add_argument('--ext', default='*.jpg')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--bgr-conv1', action='store_true', help='the weights expect BGR input: flip conv1, see load_npz')
    ap.add_argument('--mean', type=float, nargs=3, default=[float(x) for x in channel_mean],
                    help='per-channel mean in the order of the image channels')
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--dtype', choices=('float32', 'float16'), default='float32', help='container of the .npy files')
    a = ap.parse_args(argv)
    if a.size < 1 or a.batch < 1:
        ap.error('--size and --batch must be positive')
    return a


def main(argv=None):
    a = parse_args(argv)
    weights = load_npz(a.weights, bgr_conv1=a.bgr_conv1)
    net = ResNetRes5c(max_N=a.batch, max_H=a.size, max_W=a.size, channel_mean=a.mean, device=a.device)
    net.load_weights(weights)
    n = extract_dataset_res5c(a.images, a.out, a.ext, net=net, size=a.size, batch_size=a.batch, verbose=True, dtype=a.dtype)
    print('wrote %d files to %s' % (n, a.out))


if __name__ == '__main__':
    main()
