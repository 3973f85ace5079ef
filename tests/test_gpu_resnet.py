"""ResNet-152 res5c features on the device (include/n2nmn.h section 10, n2nmn_amd/resnet.py) against
tests/resnet_oracle.py: a torch CPU restatement of the published network working from the RAW weights
(convolution, batch-norm, scale), while the device runs the folded ones.

Error measure: max|out - ref64| / max|ref64| per compared tensor.  Yardstick: e32, the same measure for the
oracle run in fp32 on the same inputs.  Bound: 4 * e32 + 1e-6 -- the factor covers a different summation order
over K up to 4608 and the fold-then-convolve rounding; the floor is for tensors whose fp32 oracle happens to be
exact.  Max-pools are compared for equality.  Measured ratios err / e32 on an MI355X are in
profiles/resnet_parity.md.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_oracle as O
from n2nmn_amd import _lib, resnet

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 1e-6
SHALLOW = (2, 2, 1, 1)


def within(tag, dev, r64, r32):
    """(ok, line): the device tensor against the fp64 oracle, bounded by the fp32 oracle's own error"""
    err, e32 = O.rel_err(dev, r64), O.rel_err(r32, r64)
    bound = FACTOR * e32 + FLOOR
    line = '%-22s %-18s err %.3e  e32 %.3e  ratio %5.2f  bound %.3e' % (
        tag, tuple(np.shape(dev)), err, e32, err / e32 if e32 > 0 else float('nan'), bound)
    print(line)
    return err <= bound, line


def ref_conv(x, w, b, stride, pad, dt, residual=None, relu=True):
    """NHWC numpy -> NHWC numpy on the CPU in dtype dt; w HWIO"""
    y = F.conv2d(torch.as_tensor(x).to(dt).permute(0, 3, 1, 2), torch.as_tensor(w).to(dt).permute(3, 2, 0, 1),
                 torch.as_tensor(b).to(dt), stride=stride, padding=pad)
    if residual is not None:
        y = y + torch.as_tensor(residual).to(dt).permute(0, 3, 1, 2)
    if relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# ---- single operations --------------------------------------------------------------------------------
@pytest.mark.parametrize('N,H,W,dtype', [(1, 37, 50, 'uint8'), (2, 64, 64, 'float32')])
def test_stem(N, H, W, dtype):
    rs = np.random.RandomState(H)
    im = rs.randint(0, 256, size=(N, H, W, 3)).astype(dtype)
    w = (rs.randn(7, 7, 3, 64) * np.sqrt(2.0 / 147)).astype(np.float32)
    b = (rs.randn(64) * 0.1).astype(np.float32)
    x = im.astype(np.float64) - resnet.channel_mean.astype(np.float64)
    r64, r32 = ref_conv(x, w, b, 2, 3, torch.float64), ref_conv(x, w, b, 2, 3, torch.float32)
    got = resnet.stem_conv(im, w, b).cpu().numpy()
    assert got.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    ok, line = within('stem', got, r64, r32)
    assert ok, line
    # the border on its own: the mean is subtracted before the padding
    border = np.ones(got.shape[1:3], bool)
    border[2:-2, 2:-2] = False
    assert np.abs(got - r64)[:, border].max() / np.abs(r64).max() <= FACTOR * O.rel_err(r32, r64) + FLOOR


@pytest.mark.parametrize('H', [7, 8])
@pytest.mark.parametrize('W', [9, 10])
def test_pool_all_parities(H, W):
    """all-negative input: a halo zero taking part in the clipped last window would win"""
    x = -(np.random.RandomState(H * 16 + W).rand(2, H, W, 64).astype(np.float32) + 0.5)
    got = resnet.max_pool_3x3_s2(x).cpu().numpy()
    ref = O.pool1(torch.as_tensor(x).double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    assert got.shape == ref.shape == (2, int(np.ceil((H - 3) / 2)) + 1, int(np.ceil((W - 3) / 2)) + 1, 64)
    assert (got < 0).all() and np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize('fused', ['plain', 'relu', 'residual', 'residual_relu'])
@pytest.mark.parametrize('H,W', [(5, 7), (8, 8)])
@pytest.mark.parametrize('Cin,Cout', [(ci, co) for ci in (64, 256) for co in (64, 256, 2048)])
@pytest.mark.parametrize('stride', [1, 2])
def test_conv1x1(stride, Cin, Cout, H, W, fused):
    """N = 3: 105 / 192 output rows at stride 1 (less than a row tile / a ragged second one), 36 / 48 at stride 2;
    5 x 7 is the odd extent of stride 2; Cout 64 is half a column tile, 2048 sixteen of them"""
    N = 3
    rs = np.random.RandomState(stride * 7 + Cin + Cout + H)
    x = rs.randn(N, H, W, Cin).astype(np.float32)
    w = (rs.randn(1, 1, Cin, Cout) * np.sqrt(2.0 / Cin)).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = rs.randn(N, ho, wo, Cout).astype(np.float32) if 'residual' in fused else None
    relu = 'relu' in fused
    r64 = ref_conv(x, w, b, stride, 0, torch.float64, res, relu)
    r32 = ref_conv(x, w, b, stride, 0, torch.float32, res, relu)
    got = resnet.conv1x1(x, w, b, stride=stride, residual=res, relu=relu).cpu().numpy()
    assert got.shape == (N, ho, wo, Cout)
    if not relu:
        assert (got < 0).any()
    ok, line = within('1x1 s%d %d->%d' % (stride, Cin, Cout), got, r64, r32)
    assert ok, line


# ---- the shallow net: every layer -------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shallow():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    raw = resnet.synthetic_weights(0, SHALLOW, 64)
    im = np.random.RandomState(5).randint(0, 256, size=(2, 70, 102, 3)).astype(np.uint8)
    net = resnet.ResNetRes5c(max_N=2, max_H=70, max_W=102, blocks=SHALLOW, base_width=64)
    net.load_weights(raw)
    r64, r32 = O.forward(im, raw, SHALLOW, torch.float64), O.forward(im, raw, SHALLOW, torch.float32)
    yield net, raw, im, r64, r32
    net.close()


def test_shallow_net_every_layer(shallow):
    net, raw, im, r64, r32 = shallow
    out = net.forward(im)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == resnet.res5c_shape(2, 70, 102) == (2, 3, 4, 2048)
    names = ['conv1', 'pool1'] + resnet.layer_names(SHALLOW)[1:]
    assert sorted(names) == sorted(r64)
    bad = []
    for name in names:
        ok, line = within(name, net.layer(name).cpu().numpy(), r64[name], r32[name])
        if not ok:
            bad.append(line)
    assert not bad, 'first wrong layer: ' + bad[0]
    last = names[-1]
    assert np.array_equal(net.layer(last).cpu().numpy(), out.cpu().numpy())
    assert np.array_equal(net.layer('res5a').cpu().numpy(), out.cpu().numpy())      # the block's own name
    assert np.array_equal(net.forward(im).cpu().numpy(), out.cpu().numpy())         # after the layer re-runs
    ok, line = within('forward', out.cpu().numpy(), r64[last], r32[last])
    assert ok, line


def test_uint8_and_float32_inputs_agree_bitwise(shallow):
    net, raw, im, r64, r32 = shallow
    a = net.forward(im).cpu().numpy()
    b = net.forward(im.astype(np.float32)).cpu().numpy()
    assert np.array_equal(a, b)


def test_smaller_batch_and_image_on_the_same_handle(shallow):
    net, raw, im, r64, r32 = shallow
    full = net.forward(torch.as_tensor(im).cuda()).cpu().numpy()
    one = net.forward(im[1:2]).cpu().numpy()                   # N = 1 on the max_N = 2 handle
    assert np.array_equal(one, full[1:2])
    small = im[:1, :37, :50]                                   # H, W below the maxima: other extents at every level
    got = net.forward(small).cpu().numpy()
    s64, s32 = O.forward(small, raw, SHALLOW, torch.float64), O.forward(small, raw, SHALLOW, torch.float32)
    ok, line = within('1 x 37 x 50', got, s64['res5a_branch2c'], s32['res5a_branch2c'])
    assert ok, line
    assert np.array_equal(net.forward(im).cpu().numpy(), full)  # and back


def test_errors_name_the_problem(shallow):
    net, raw, im, r64, r32 = shallow
    with pytest.raises(ValueError, match='exceeds'):
        net.forward(np.zeros((3, 70, 102, 3), np.uint8))
    with pytest.raises(ValueError, match='exceeds'):
        net.forward(np.zeros((1, 71, 102, 3), np.uint8))
    with pytest.raises(KeyError, match='fc1000'):
        net.layer('fc1000')
    folded = resnet.fold_batchnorm(raw)
    with pytest.raises(KeyError, match='res9z_branch2a'):
        net.load_weights(dict(folded, **{'res9z_branch2a/weights': folded['conv1/weights']}))
    bad = dict(folded)
    bad['res3a_branch2a/weights'] = folded['res3b_branch2a/weights']     # [1,1,512,128] where [1,1,256,128] belongs
    with pytest.raises(ValueError, match=r'res3a_branch2a/weights has shape \[1, 1, 512, 128\], expected \[1, 1, 256, 128\]'):
        net.load_weights(bad)
    net.load_weights(raw)                                                # (the handle stays usable)
    assert np.array_equal(net.forward(im).cpu().numpy(), net.forward(im).cpu().numpy())
    fresh = resnet.ResNetRes5c(max_N=1, max_H=32, max_W=32, blocks=(1, 1, 1, 1), base_width=32)
    with pytest.raises(_lib.N2nmnError, match='N2NMN_ENOWEIGHT'):
        fresh.forward(np.zeros((1, 32, 32, 3), np.uint8))
    fresh.close()
    with pytest.raises(ValueError, match='base_width'):
        resnet.ResNetRes5c(max_N=1, max_H=32, max_W=32, blocks=(1, 1, 1, 1), base_width=48)


def test_res5c_feeds_vqa_engine_without_host_copy(shallow):
    """the shallow net's (2, 3, 4, 2048) grid on the device -> VQAEngine.forward as image_feat_batch; the logits
    equal those of the same grid handed over as a host array"""
    from n2nmn_amd import synth, vqa
    net, raw, im, r64, r32 = shallow
    feat = net.forward(im)
    d = vqa.VQADims(N=2, H=3, W=4, D=2048, num_vocab_txt=200, num_choices=64)
    assert feat.is_cuda and tuple(feat.shape) == (d.N, d.H, d.W, d.D)
    feat = feat / feat.max()                                   # (still on the device) the scale of trained features
    eng = vqa.VQAEngine(d)
    eng.load_weights(synth.make_weights_from_shapes(vqa.vqa_variable_shapes(d), seed=0))
    rng = np.random.default_rng(3)
    lens = np.array([5, d.T_encoder], np.int32)
    seq = rng.integers(0, d.num_vocab_txt, size=(d.T_encoder, d.N)).astype(np.int32)
    seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
    gt = np.ascontiguousarray(np.array([synth.module_list2tokens(t, d.T_decoder, vqa.VQA_MODULE_NAMES) for t in
                                        (['_Find', '_Describe'], ['_Find', '_Transform', '_Find', '_And', '_Describe'])],
                                       np.int32).T)
    batch = dict(input_seq_batch=seq, seq_length_batch=lens)
    s_dev, _, ok = eng.forward(dict(batch, image_feat_batch=feat), use_gt_layout=True, gt_layout=gt)
    s_dev = s_dev.cpu().numpy().copy()
    s_host, _, _ = eng.forward(dict(batch, image_feat_batch=feat.cpu().numpy()), use_gt_layout=True, gt_layout=gt)
    s_host = s_host.cpu().numpy()
    assert np.asarray(ok).all() and np.isfinite(s_dev).all() and np.abs(s_dev).max() > 0
    assert np.array_equal(s_dev, s_host)


def test_extract_dataset_res5c(shallow, tmp_path):
    from PIL import Image
    net, raw, im, r64, r32 = shallow
    src, dst = tmp_path / 'train2014', tmp_path / 'resnet_res5c' / 'train2014'
    src.mkdir()
    Image.fromarray(im[0, :64, :64]).save(str(src / 'COCO_train2014_000000000009.png'))
    Image.fromarray(im[1]).save(str(src / 'COCO_train2014_000000000025.png'))      # 70 x 102: resized
    assert resnet.extract_dataset_res5c(str(src), str(dst), '*.png', net=net, size=64) == 2
    a = np.load(str(dst / 'COCO_train2014_000000000009.npy'))
    assert a.shape == (1, 2, 2, 2048) and a.dtype == np.float32
    assert np.array_equal(a, net.forward(im[:1, :64, :64]).cpu().numpy())
    assert np.load(str(dst / 'COCO_train2014_000000000025.npy')).shape == (1, 2, 2, 2048)
    assert resnet.extract_dataset_res5c(str(src), str(dst), '*.png', net=net, size=64) == 0    # existing files stay


# ---- full depth, once ---------------------------------------------------------------------------------------
def test_full_depth_152():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    blocks = (3, 8, 36, 3)
    raw = resnet.synthetic_weights(0, blocks, 64)
    im = np.random.RandomState(9).randint(0, 256, size=(1, 64, 96, 3)).astype(np.uint8)
    net = resnet.ResNetRes5c(max_N=1, max_H=64, max_W=96)
    net.load_weights(raw)
    out = net.forward(im)
    assert tuple(out.shape) == (1, 2, 3, 2048)
    r64, r32 = O.forward(im, raw, blocks, torch.float64), O.forward(im, raw, blocks, torch.float32)
    assert len(r64) == 155 + 1
    bad = []
    for name in ('res2c_branch2c', 'res3b7_branch2b', 'res4b20_branch2a', 'res5c_branch2c'):
        ok, line = within(name, net.layer(name).cpu().numpy(), r64[name], r32[name])
        if not ok:
            bad.append(line)
    ok, line = within('forward (res5c)', out.cpu().numpy(), r64['res5c_branch2c'], r32['res5c_branch2c'])
    net.close()
    assert not bad and ok, bad + [line]
