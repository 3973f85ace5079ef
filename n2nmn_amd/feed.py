"""Compact feature feed (include/n2nmn.h section 11): image features cross the link as fp16 and / or one row
per image, and `n2nmn_features_expand` widens / gathers them into the fp32 grid every kernel reads.

    slot[n] = widen(src[index[n]])

A COMPACT batch is a reader batch whose `image_feat_batch` is float16 and / or which carries an
`image_index_batch` (int32 [nb]) into an `image_feat_batch` of U <= nb rows.  `Engine.features`,
`SuperBucket.fill`, `DeviceFeeder` and `VQAEngine.fill_slab` take it; `narrow` is the way back (extractors).
Torch is plumbing only: the arithmetic (the conversions) runs in libn2nmn_hip.so.
"""
from __future__ import annotations

import numpy as np

from . import _lib

FEAT_F32, FEAT_F16 = 0, 1          # N2NMN_FEAT_F32 / N2NMN_FEAT_F16


def is_half(x) -> bool:
    """is `x` (numpy array or torch tensor) stored as IEEE half"""
    dt = getattr(x, 'dtype', None)
    return dt is not None and str(dt).rsplit('.', 1)[-1] == 'float16'


def is_compact(batch) -> bool:
    return batch.get('image_index_batch') is not None or is_half(batch['image_feat_batch'])


def half_requested(dtype) -> bool:
    """None / 'float32' -> False, 'float16' (name, numpy or torch dtype) -> True, anything else ValueError"""
    if dtype is None:
        return False
    name = str(getattr(dtype, '__name__', dtype)).rsplit('.', 1)[-1]
    if name == 'float16':
        return True
    if name == 'float32':
        return False
    raise ValueError("feature dtype must be None, 'float32' or 'float16', got %r" % (dtype,))


def check_index(index, rows: int, n=None):
    """A HOST index (numpy array, list, CPU tensor) is checked here, before any device call: 1-D, of `n`
    entries when n is given, every value in [0, rows).  Returns it as contiguous int32; a device tensor is
    returned as it is (the kernel writes zeros for a row it cannot find and reads nothing outside the source)."""
    if hasattr(index, 'is_cuda'):
        if index.is_cuda:
            if index.dim() != 1 or (n is not None and index.shape[0] != n):
                raise ValueError('image index must hold %s entries, got shape %s' % (n, tuple(index.shape)))
            return index
        index = index.numpy()
    a = np.asarray(index)
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError('image index must be 1-D%s, got shape %s'
                         % ('' if n is None else ' with %d entries' % n, a.shape))
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError('image index must be integers, got %s' % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= rows):
        raise ValueError('image index outside [0, %d): min %d, max %d' % (rows, int(a.min()), int(a.max())))
    return np.ascontiguousarray(a, np.int32)


def expand(src, index, dst, D=None):
    """dst[n, ..., :D] = float(src[index[n] if index is not None else n]) on dst's device and the current
    stream.  src: contiguous device tensor [rows, ..., D], float16 or float32; index: int32 device tensor
    [N] or None; dst: float32 device tensor [N, ..., Dp >= D], contiguous (channels D .. Dp-1 stay as they are)."""
    import torch
    if src.dtype not in (torch.float16, torch.float32) or dst.dtype != torch.float32:
        raise ValueError('expand: float16 / float32 source and float32 destination, got %s -> %s'
                         % (src.dtype, dst.dtype))
    if not (src.is_contiguous() and dst.is_contiguous()) or src.device != dst.device or not src.is_cuda:
        raise ValueError('expand: source and destination must be contiguous tensors on one GPU')
    D = int(src.shape[-1] if D is None else D)
    N = int(dst.shape[0])
    if src.dim() < 2 or src.dim() != dst.dim() or src.shape[-1] != D or dst.shape[-1] < D or \
            tuple(src.shape[1:-1]) != tuple(dst.shape[1:-1]):
        raise ValueError('expand: source %s does not fit destination %s' % (tuple(src.shape), tuple(dst.shape)))
    pixels = 1
    for e in src.shape[1:-1]:
        pixels *= int(e)
    if index is None:
        if N > src.shape[0]:
            raise ValueError('expand: %d destination rows from %d source rows needs an index' % (N, src.shape[0]))
    elif index.dtype != torch.int32 or not index.is_contiguous() or index.device != dst.device or \
            tuple(index.shape) != (N,):
        raise ValueError('expand: the index must be a contiguous int32 [%d] tensor on the destination device' % N)
    with torch.cuda.device(dst.device):
        _lib.check(_lib.lib().n2nmn_features_expand(
            src.data_ptr(), FEAT_F16 if src.dtype == torch.float16 else FEAT_F32, int(src.shape[0]),
            None if index is None else index.data_ptr(), N, pixels, D, int(dst.shape[-1]), dst.data_ptr(),
            torch.cuda.current_stream(dst.device).cuda_stream))
    return dst


def narrow(src):
    """float32 device tensor -> float16 device tensor of the same shape, round to nearest even
    (n2nmn_features_narrow), on the current stream"""
    import torch
    if src.dtype != torch.float32 or not src.is_cuda:
        raise ValueError('narrow: a float32 device tensor, got %s on %s' % (src.dtype, src.device))
    src = src.contiguous()
    out = torch.empty(src.shape, dtype=torch.float16, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().n2nmn_features_narrow(src.data_ptr(), src.numel(), out.data_ptr(),
                                                    torch.cuda.current_stream(src.device).cuda_stream))
    return out
