"""Compact feature feed on the device (include/n2nmn.h section 11, csrc/kernels_feed.hip): n2nmn_features_expand
(slot[n] = widen(src[index[n]])) and n2nmn_features_narrow, and every face that takes a compact batch -- Engine,
SuperBucket / DeviceFeeder, VQAEngine.fill_slab, the two extractors.

Every comparison is BITWISE: widening a half is exact, numpy's astype(float16) is round-to-nearest-even like the
kernel's, and both sides of each end-to-end comparison run the same kernels on the same fp32 values.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import data_reader_cases as DC  # noqa: E402

from n2nmn_amd import _lib, feed, synth
from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def off_by_one(a):
    """a device copy of `a` whose first element sits one element behind a 16-byte boundary, inside a zeroed
    buffer (the returned tensor's `_base`) with 7 more elements behind it"""
    buf = torch.zeros(a.size + 8, dtype=torch.as_tensor(a).dtype, device='cuda')
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.as_tensor(a))
    assert t.data_ptr() % 16 == a.dtype.itemsize and t.is_contiguous() and t._base is buf
    return t


# ---- expand -------------------------------------------------------------------------------------------------
def test_expand_widens_every_half_exactly():
    src = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(16, 4, 1024)
    want = src.astype(np.float32)
    nan = np.isnan(src)
    assert int(nan.sum()) == 2046 and np.array_equal(nan, np.isnan(want))
    dst = torch.full((16, 4, 1024), 7.0, dtype=torch.float32, device='cuda')
    feed.expand(torch.as_tensor(src).cuda(), None, dst)
    got = dst.cpu().numpy()
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])       # subnormals, signed zeros, infinities included
    assert np.isnan(got[nan]).all() and int(np.isnan(got).sum()) == 2046


GEOMETRIES = [
    # (pixels, D, stride, N): 16-byte path with a gap behind every pixel; D no multiple of 8 (fp16: one element per
    # lane, fp32: 16-byte path); one element per lane for both; more rows than the grid's 2048 workgroups
    (3, 8, 12, 13), (3, 20, 20, 13), (2, 7, 7, 13), (1, 8, 8, 4100)]
SENTINEL = np.float32(-1234.5)


def gather_case(pixels, D, stride, N, dtype, seed=0):
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal((5, pixels, D)) * 3).astype(dtype)
    src[0, 0, 0], src[4, -1, -1] = -0.0, 6.1e-5            # a signed zero; in half a subnormal
    index = np.array([3, 0, 0, 4, 1, 3, 3, 0, 4, 1, 0, 3, 4], np.int32)          # row 2 is never used
    index = index[rng.integers(0, 13, size=N)] if N != 13 else index
    assert 2 not in index and set(index) == {0, 1, 3, 4}
    want = np.full((N, pixels, stride), SENTINEL, np.float32)
    want[..., :D] = src.astype(np.float32)[index]
    return src, index, want


@pytest.mark.parametrize('dtype', [np.float16, np.float32])
@pytest.mark.parametrize('pixels,D,stride,N', GEOMETRIES)
def test_expand_gathers_rows_into_a_strided_destination(pixels, D, stride, N, dtype):
    src, index, want = gather_case(pixels, D, stride, N, dtype)
    dst = torch.full(want.shape, float(SENTINEL), dtype=torch.float32, device='cuda')
    feed.expand(torch.as_tensor(src).cuda(), torch.as_tensor(index).cuda(), dst, D=D)
    assert same_bits(dst.cpu().numpy(), want)
    # without an index: the plain widening / copy of the first rows
    dst.fill_(float(SENTINEL))
    feed.expand(torch.as_tensor(src).cuda(), None, dst[:4], D=D)
    want4 = np.full((4, pixels, stride), SENTINEL, np.float32)
    want4[..., :D] = src[:4].astype(np.float32)
    assert same_bits(dst[:4].cpu().numpy(), want4) and (dst[4:] == float(SENTINEL)).all()


@pytest.mark.parametrize('dtype', [np.float16, np.float32])
def test_expand_off_16_byte_alignment(dtype):
    src, index, want = gather_case(3, 8, 12, 13, dtype, seed=1)
    s, dst = off_by_one(src), off_by_one(np.full(want.shape, SENTINEL, np.float32))
    feed.expand(s, torch.as_tensor(index).cuda(), dst, D=8)
    assert same_bits(dst.cpu().numpy(), want)
    whole = dst._base.cpu().numpy()                                  # nothing in front of or behind the destination
    assert whole[0] == 0 and not whole[1 + want.size:].any()


def test_expand_and_narrow_argument_checks():
    L = _lib.lib()
    assert L.n2nmn_features_expand(None, feed.FEAT_F16, 0, None, 0, 3, 8, 8, None, None) == 0      # N == 0
    assert L.n2nmn_features_narrow(None, 0, None, None) == 0
    x = torch.zeros(64, dtype=torch.float32, device='cuda')
    p = x.data_ptr()
    for args, msg in (((p, 7, 2, None, 2, 2, 4, 4, p, None), 'unknown src_dtype'),
                      ((p, 0, 2, None, 2, 2, 4, 3, p, None), 'dst_pixel_stride < D'),
                      ((p, 0, 2, None, -1, 2, 4, 4, p, None), 'negative'),
                      ((None, 0, 2, None, 2, 2, 4, 4, p, None), 'null src'),
                      ((p, 0, 2, None, 2, 2, 4, 4, None, None), 'null dst'),
                      ((p, 0, 2, None, 3, 2, 4, 4, p, None), 'must not exceed src_rows')):
        with pytest.raises(ValueError, match=msg):
            _lib.check(L.n2nmn_features_expand(*args))
    with pytest.raises(ValueError, match='negative'):
        _lib.check(L.n2nmn_features_narrow(p, -1, p, None))
    with pytest.raises(ValueError, match='null'):
        _lib.check(L.n2nmn_features_narrow(None, 8, p, None))
    torch.cuda.synchronize()
    assert (x == 0).all()


# ---- narrow -------------------------------------------------------------------------------------------------
def narrow_cases():
    """float32 inputs whose rounding to half is decided at the last bit: every midpoint between consecutive
    non-negative finite halves, each one fp32 ulp up and down, their mirror images, the ends of the range"""
    h = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)       # 0 .. 65504, ascending
    mid64 = (h[:-1] + h[1:]) / 2
    mid = mid64.astype(np.float32)
    assert mid.shape == (31743,) and np.array_equal(mid.astype(np.float64), mid64)    # exactly representable
    even = np.where(np.arange(31743) % 2 == 0, np.arange(31743), np.arange(31743) + 1).astype(np.uint16)
    assert np.array_equal(mid.astype(np.float16).view(np.uint16), even)                # numpy: ties to even
    up, down = np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))
    assert np.array_equal(up.astype(np.float16).view(np.uint16), np.arange(1, 31744, dtype=np.uint16))
    assert np.array_equal(down.astype(np.float16).view(np.uint16), np.arange(31743, dtype=np.uint16))
    tiny = np.float32(2.0 ** -25)
    with np.errstate(over='ignore'):
        special = np.array([65504, 65519.996, 65520, tiny, np.nextafter(tiny, np.float32(1)), 1e-40, -1e-40,
                            np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0], np.float32)
        want = special.astype(np.float16)
    assert want[1] == 65504 and np.isinf(want[2]) and want[3] == 0 and want[4] == np.float16(2.0 ** -24)
    assert bits(want)[5] == 0 and bits(want)[6] == 0x8000 and np.isnan(want[9])
    x = np.concatenate([mid, up, down, -mid, -up, -down, special])
    assert x.size % 8 != 0
    return x


def test_narrow_rounds_to_nearest_even_like_numpy():
    x = narrow_cases()
    with np.errstate(over='ignore'):
        want = x.astype(np.float16)
    nan = np.isnan(want)
    assert int(nan.sum()) == 1
    for dev in (torch.as_tensor(x).cuda(), off_by_one(x)):           # 8 per lane + tail; one element per lane
        got = feed.narrow(dev)
        assert got.dtype == torch.float16 and got.shape == dev.shape
        got = got.cpu().numpy()
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
        assert np.isnan(got[nan]).all()
    # the destination off alignment too (the entry point itself: narrow() allocates an aligned one)
    dev = torch.as_tensor(x).cuda()
    out = torch.zeros(x.size + 8, dtype=torch.float16, device='cuda')
    _lib.check(_lib.lib().n2nmn_features_narrow(dev.data_ptr(), x.size, out[1:].data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    assert np.array_equal(bits(got[1:1 + x.size])[~nan], bits(want)[~nan])
    assert bits(got)[0] == 0 and not bits(got)[1 + x.size:].any()


# ---- Engine -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_engine():
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    d = Dims(N=8)
    asm = Assembler(list(CLEVR_MODULE_NAMES))
    eng = Engine(d, asm)
    w = synth.make_weights(d, seed=0)
    eng.load_weights(w)
    return eng, d, asm, w


def run_forward(eng, batch, **kw):
    s, t, v = eng.forward(batch, **kw)
    return s.cpu().numpy().copy(), np.asarray(t).copy(), np.asarray(v).copy()


def test_engine_forward_takes_half_features_and_an_image_index(small_engine):
    eng, d, asm, w = small_engine
    batch = synth.make_inputs(d, seed=11)
    gt = synth.template_layout_batch(d)
    feat16 = batch['image_feat_batch'].astype(np.float16)
    index = np.array([2, 0, 0, 1, 2, 2, 1, 0], np.int32)
    for kw in (dict(use_gt_layout=True, gt_layout=gt), dict(), dict(host_assemble=True)):
        # fp16 features, one row per question
        want = run_forward(eng, dict(batch, image_feat_batch=feat16.astype(np.float32)), **kw)
        got = run_forward(eng, dict(batch, image_feat_batch=feat16), **kw)
        assert all(same_bits(g, x) for g, x in zip(got, want))
        # U = 3 rows and an index, fp16 and fp32 containers
        want = run_forward(eng, dict(batch, image_feat_batch=feat16[:3].astype(np.float32)[index]), **kw)
        for rows in (feat16[:3], feat16[:3].astype(np.float32), torch.as_tensor(feat16[:3]).cuda()):
            got = run_forward(eng, dict(batch, image_feat_batch=rows, image_index_batch=index), **kw)
            assert all(same_bits(g, x) for g, x in zip(got, want))
    out = eng.features(feat16[:3], index)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (8, d.H, d.W, d.D)
    assert same_bits(out.cpu().numpy(), feat16[:3].astype(np.float32)[index])
    plain = torch.as_tensor(batch['image_feat_batch']).cuda()
    assert eng.features(plain) is plain                              # the default path is _dev: nothing runs
    with pytest.raises(ValueError, match='8 entries'):
        eng.forward(dict(batch, image_feat_batch=feat16[:3], image_index_batch=index[:5]))


# ---- reader -> DeviceFeeder -> SuperBucket ------------------------------------------------------------------
def shared_imdb(root, d, rounded):
    """the 37-question imdb of the feeder test with questions 3j, 3j+1, 3j+2 asking about one image; rounded: the
    feature files rewritten as astype(float16).astype(float32)"""
    imdb, params = DC.build(root, 'clevr', n=37, H=d.H, W=d.W, D=d.D)
    for i, info in enumerate(imdb):
        info['feature_path'] = imdb[3 * (i // 3)]['feature_path']
    if rounded:
        for path in sorted({info['feature_path'] for info in imdb}):
            np.save(path, np.load(path).astype(np.float16).astype(np.float32))
    return imdb, params


def run_feeder(buckets, imdb, params, check=None, **options):
    from n2nmn_amd.data_reader import DataReader, DeviceFeeder
    d, asm = buckets[0].dims, buckets[0].engine.assembler
    params = dict(params, batch_size=d.N, T_encoder=d.T_encoder, T_decoder=d.T_decoder, assembler=asm, **options)
    feeder = DeviceFeeder(DataReader(None, imdb=imdb, shuffle=False, one_pass=True, **params), buckets,
                          use_gt_layout=True)
    logits, sizes, first = [], [], 0
    for group in feeder.groups():
        feeder.wait(group)
        bk = group.bucket
        bk.run(use_gt_layout=True)
        sizes.append(len(group.batches))
        for k, b in enumerate(group.batches):
            nb = b['seq_length_batch'].shape[0]
            sc, tok, val = bk.result(k)
            logits.append((sc[:nb].cpu().numpy(), val[:nb].cpu().numpy()))
            if check is not None:
                check(b, bk.slot(k)['image_feat_batch'][:nb].cpu().numpy(), imdb[first:first + nb])
            first += nb
    assert sizes == [2, 2, 1] and first == 37
    feeder.reader.close()
    return logits


def test_feeder_ships_half_rows_per_image_and_expands_them_on_the_copy_stream(tmp_path):
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.superbucket import SuperBucket
    d = Dims(N=8)
    asm = Assembler(list(CLEVR_MODULE_NAMES))
    w = synth.make_weights(d, seed=0)
    buckets = [SuperBucket(d, asm, K=2), SuperBucket(d, asm, K=2)]
    for bk in buckets:
        bk.load_weights(w)
    imdb, params = shared_imdb(str(tmp_path / 'a'), d, rounded=False)
    imdb_r, params_r = shared_imdb(str(tmp_path / 'b'), d, rounded=True)

    def check(b, slot_rows, infos):
        paths = []
        for info in infos:
            if info['feature_path'] not in paths:
                paths.append(info['feature_path'])
        feat, index = b['image_feat_batch'], b['image_index_batch']
        assert feat.dtype == np.float16 and feat.shape == (len(paths), d.H, d.W, d.D)
        assert index.dtype == np.int32 and [paths[j] for j in index] == [info['feature_path'] for info in infos]
        want = np.concatenate([np.load(info['feature_path']).astype(np.float16).astype(np.float32) for info in infos])
        assert same_bits(slot_rows, want)

    got = run_feeder(buckets, imdb, params, check, feature_dtype='float16', dedupe_features=True)

    def check_plain(b, slot_rows, infos):
        assert 'image_index_batch' not in b and b['image_feat_batch'].dtype == np.float32
        assert same_bits(slot_rows, np.ascontiguousarray(b['image_feat_batch']))

    want = run_feeder(buckets, imdb_r, params_r, check_plain)
    assert [x[0].shape[0] for x in want] == [8, 8, 8, 8, 5]
    for (gs, gv), (ws, wv) in zip(got, want):
        assert same_bits(gs, ws) and np.array_equal(gv, wv) and gv.all()
    # each option alone lands on the same logits (files already rounded: the half container loses nothing)
    for options in (dict(feature_dtype='float16'), dict(dedupe_features=True)):
        for (gs, gv), (ws, wv) in zip(run_feeder(buckets, imdb_r, params_r, None, **options), want):
            assert same_bits(gs, ws) and np.array_equal(gv, wv)


def test_superbucket_fill_takes_a_compact_batch(small_engine):
    from n2nmn_amd.superbucket import SuperBucket
    eng, d, asm, w = small_engine
    sb = SuperBucket(d, asm, K=2, engine=None)
    sb.load_weights(w)
    gt = synth.template_layout_batch(d)
    a, b = synth.make_inputs(d, seed=21), synth.make_inputs(d, seed=22)
    a16, b16 = a['image_feat_batch'].astype(np.float16), b['image_feat_batch'].astype(np.float16)
    index = np.array([1, 1, 0, 2, 2, 2, 0, 1], np.int32)
    sb.fill(0, dict(a, image_feat_batch=a16.astype(np.float32)), gt)
    sb.fill(1, dict(b, image_feat_batch=b16[:3].astype(np.float32)[index]), gt)
    want = sb.run(use_gt_layout=True)[0].cpu().numpy().copy()
    sb.image_feat.zero_()
    sb.fill(0, dict(a, image_feat_batch=a16), gt)
    sb.fill(1, dict(b, image_feat_batch=b16[:3], image_index_batch=index), gt)
    assert same_bits(sb.slot(1)['image_feat_batch'].cpu().numpy(), b16[:3].astype(np.float32)[index])
    assert same_bits(sb.run(use_gt_layout=True)[0].cpu().numpy(), want)
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
        sb.fill(1, dict(b, image_feat_batch=b16[:3], image_index_batch=index + 1), gt)


# ---- models_vqa ---------------------------------------------------------------------------------------------
def test_vqa_fill_slab_keeps_the_coordinate_channels():
    from n2nmn_amd import vqa
    import test_gpu_vqa as TV
    d = vqa.VQADims(N=TV.NQ)
    eng = vqa.VQAEngine(d)
    eng.load_weights(synth.make_weights_from_shapes(vqa.vqa_variable_shapes(d), seed=0))
    batch = TV._batch(d, 3)
    gt = TV._gt(eng, d)
    rows16 = batch['image_feat_batch'][:5].astype(np.float16)
    index = (np.arange(d.N) * 7 % 5).astype(np.int32)
    expanded = rows16.astype(np.float32)[index]
    Dp = eng.idims.D
    assert Dp > d.D + 2

    ref = eng.feature_slab(d.N)
    coords = ref[..., d.D:].cpu().numpy().copy()
    ref[..., :d.D].copy_(torch.as_tensor(expanded))
    want, _, ok = eng.forward(dict(batch, image_feat_batch=ref), use_gt_layout=True, gt_layout=gt)
    want = want.cpu().numpy().copy()
    assert np.asarray(ok).all()

    slab = eng.feature_slab(d.N)
    out = eng.fill_slab(slab, rows16, index)
    assert out.data_ptr() == slab.data_ptr() and tuple(out.shape) == (d.N, d.H, d.W, Dp)
    assert same_bits(slab[..., d.D:].cpu().numpy(), coords)           # coordinate channels and padding: untouched
    assert same_bits(slab[..., :d.D].cpu().numpy(), expanded)
    got, _, _ = eng.forward(dict(batch, image_feat_batch=slab), use_gt_layout=True, gt_layout=gt)
    assert same_bits(got.cpu().numpy(), want)
    # the per-pass route (features_with_coords) takes the same compact batch
    got, _, _ = eng.forward(dict(batch, image_feat_batch=rows16, image_index_batch=index), use_gt_layout=True,
                            gt_layout=gt)
    assert same_bits(got.cpu().numpy(), want)
    # fp32 rows without an index into part of a slab; rows behind them stay
    eng.fill_slab(slab[2:], batch['image_feat_batch'][:3])
    assert same_bits(slab[2:5, ..., :d.D].cpu().numpy(), batch['image_feat_batch'][:3])
    assert same_bits(slab[5:, ..., :d.D].cpu().numpy(), expanded[5:]) and same_bits(slab[..., d.D:].cpu().numpy(), coords)
    with pytest.raises(ValueError, match='feature_slab'):
        eng.fill_slab(torch.zeros((2, d.H, d.W, Dp), device='cuda'), rows16[:2])
    with pytest.raises(ValueError, match=r'outside \[0, 5\)'):
        eng.fill_slab(slab, rows16, index + 1)


# ---- extractors ---------------------------------------------------------------------------------------------
def test_vgg_pool5_narrows_on_the_device(tmp_path):
    from PIL import Image
    from n2nmn_amd import vgg_net
    g = np.load(os.path.join(HERE, 'golden', 'vgg_golden.npz'))
    im = g['images_A']                                               # (2, 34, 50, 3): the smallest of test_gpu_vgg.py
    v = vgg_net.VGGPool5(max_N=2, max_H=34, max_W=50)
    v.load_weights(vgg_net.synthetic_weights(int(g['seed'])))
    full = v.forward(im)
    half = v.forward(im, out_dtype='float16')
    assert half.is_cuda and half.dtype == torch.float16 and half.shape == full.shape
    assert same_bits(half.cpu().numpy(), full.cpu().numpy().astype(np.float16))
    assert v.forward(im, out_dtype='float32').dtype == torch.float32
    src, dst = tmp_path / 'images', tmp_path / 'vgg_pool5'
    src.mkdir()
    for i in range(2):
        Image.fromarray(im[i]).save(str(src / ('CLEVR_%d.png' % i)))
    assert vgg_net.extract_dataset_pool5(str(src), str(dst), vgg=v, dtype='float16') == 2
    for i in range(2):
        a = np.load(str(dst / ('CLEVR_%d.npy' % i)))
        assert a.dtype == np.float16 and a.shape == (1, 2, 2, 512)
        assert same_bits(a, full[i:i + 1].cpu().numpy().astype(np.float16))
    v.close()


def test_resnet_res5c_narrows_on_the_device():
    from n2nmn_amd import resnet
    import test_gpu_resnet as TR
    im = np.random.RandomState(5).randint(0, 256, size=(1, 37, 50, 3)).astype(np.uint8)
    net = resnet.ResNetRes5c(max_N=1, max_H=37, max_W=50, blocks=TR.SHALLOW, base_width=64)
    net.load_weights(resnet.synthetic_weights(0, TR.SHALLOW, 64))
    full = net.forward(im)
    half = net.forward(im, out_dtype='float16')
    assert half.is_cuda and half.dtype == torch.float16
    assert tuple(half.shape) == tuple(full.shape) == resnet.res5c_shape(1, 37, 50)
    assert same_bits(half.cpu().numpy(), full.cpu().numpy().astype(np.float16))
    net.close()
