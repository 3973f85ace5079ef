"""VGG-16 pool5 features on the device (include/n2nmn.h section 9, n2nmn_amd/vgg_net.py) against
tests/golden/vgg_golden.npz -- the reference's unmodified models_clevr/vgg_net.py run in fp64 under
oracle/tf1_stub (tests/golden/make_vgg_golden.py) -- and, layer by layer, against an fp64 torch CPU chain.

Error measure: max|out - ref| / max|ref|.  Yardstick: the fp32 torch CPU chain (conv2d(padding=1),
max_pool2d(2, 2, ceil_mode=True)) on the same inputs, NOT the code under test.  Measured against the fixture with
seed-0 synthetic weights: case A (N = 2, 34 x 50) 2.13e-06, case B (N = 1, 64 x 96) 1.57e-06.  The GPU is allowed
8 x the larger one, TOL = 1.70e-05: the margin covers the different summation order of a K-split MFMA against a
CPU dot product over 13 layers.  Per-layer and single-layer checks use the same rule with that layer's own
fp32-CPU error, computed here, as the yardstick (fp32 CPU error of case A per layer: conv1_1 2.1e-07,
conv1_2 7.6e-07, conv2_2 1.0e-06, conv3_3 2.2e-06, conv4_3 2.0e-06, conv5_3 2.1e-06).  Max-pools are exact.
Measured on an MI355X: case A 2.40e-06, case B 2.70e-06 (uint8 and float32 input alike); every layer of case A
between 0.8 x and 1.5 x its fp32-CPU error; the single-layer shapes between 1.0 x and 2.2 x.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from n2nmn_amd import tf_checkpoint, vgg_net

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vgg_golden.npz')
CPU_FP32_ERR = {'A': 2.13e-6, 'B': 1.57e-6}          # measured, see above
TOL = 8 * max(CPU_FP32_ERR.values())


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.fixture(scope='module')
def fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def weights(fixture):
    return vgg_net.synthetic_weights(int(fixture['seed']))


@pytest.fixture(scope='module')
def vgg(weights):
    """one handle for both cases: the halo geometry changes between them, back and forth"""
    v = vgg_net.VGGPool5(max_N=2, max_H=64, max_W=96)
    v.load_weights(weights)
    yield v
    v.close()


def cpu_conv(x, w, b, dt):
    """NHWC numpy -> NHWC numpy: relu(conv3x3 SAME + bias) on the CPU in dtype dt"""
    y = F.relu(F.conv2d(torch.as_tensor(x).to(dt).permute(0, 3, 1, 2), torch.as_tensor(w).to(dt).permute(3, 2, 0, 1),
                        torch.as_tensor(b).to(dt), padding=1))
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def cpu_pool(x, dt):
    y = F.max_pool2d(torch.as_tensor(x).to(dt).permute(0, 3, 1, 2), 2, 2, ceil_mode=True)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def cpu_chain(images, weights, dt):
    x = images.astype(np.float32) - vgg_net.channel_mean       # as the reference's script forms it
    acts = {}
    for name in vgg_net.LAYERS:
        x = cpu_pool(x, dt) if name.startswith('pool') else \
            cpu_conv(x, weights[name + '/weights'], weights[name + '/biases'], dt)
        acts[name] = x
    return acts


@pytest.fixture(scope='module')
def chains_A(fixture, weights):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return cpu_chain(fixture['images_A'], weights, torch.float64), cpu_chain(fixture['images_A'], weights, torch.float32)


@pytest.mark.parametrize('case', ['A', 'B'])
@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_pool5_against_reference_fixture(vgg, fixture, case, dtype):
    im = fixture['images_' + case]
    out = vgg.forward(im if dtype == 'uint8' else im.astype(np.float32))
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == fixture['pool5_' + case].shape
    err = rel_err(out.cpu().numpy(), fixture['pool5_' + case])
    print('case %s %s: rel err %.3e (fp32 CPU chain %.3e, bound %.3e)' % (case, dtype, err, CPU_FP32_ERR[case], TOL))
    assert err <= TOL


def test_every_layer_of_case_A(vgg, fixture, chains_A):
    """where an error starts: conv1_1's border pixels (mean subtracted before the padding), each pool's odd
    extent, each tile edge.  The fp64 chain itself equals the reference fixture to 1e-12."""
    c64, c32 = chains_A
    assert rel_err(c64['pool5'], fixture['pool5_A']) < 1e-12
    vgg.forward(fixture['images_A'])
    bad = []
    for name in vgg_net.LAYERS:
        got = vgg.layer(name).cpu().numpy()
        err, yard = rel_err(got, c64[name]), rel_err(c32[name], c64[name])
        print('%-8s %-18s rel err %.3e  fp32 CPU %.3e  bound %.3e' % (name, got.shape, err, yard, 8 * yard))
        if err > 8 * yard:
            bad.append((name, err, yard))
    assert not bad, bad
    # the border pixels of conv1_1 on their own: a tap outside the image contributes 0, not -mean * w
    got, ref = vgg.layer('conv1_1').cpu().numpy().astype(np.float64), c64['conv1_1']
    border = np.ones(ref.shape[1:3], bool)
    border[1:-1, 1:-1] = False
    assert np.abs(got - ref)[:, border].max() / np.abs(ref).max() <= 8 * rel_err(c32['conv1_1'], c64['conv1_1'])


@pytest.mark.parametrize('N,H,W,Cin,Cout', [
    (3, 5, 7, 64, 64),          # Cout = half a column tile; 105 rows: less than one row tile
    (3, 5, 7, 64, 128),
    (3, 5, 7, 512, 512),        # four column tiles, 144 k stages
    (1, 3, 4, 64, 64),          # N H W = 12 < 128
    (2, 9, 1, 64, 128),         # W = 1: every dx != 1 tap is halo
    (2, 9, 11, 128, 256),       # 198 rows: two row tiles, the second ragged, straddling the image boundary
])
def test_single_conv_layer_edges(N, H, W, Cin, Cout):
    rs = np.random.RandomState(N * 1000 + H * 100 + W * 10 + Cin + Cout)
    x = rs.randn(N, H, W, Cin).astype(np.float32)
    w = (rs.randn(3, 3, Cin, Cout) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    ref, c32 = cpu_conv(x, w, b, torch.float64), cpu_conv(x, w, b, torch.float32)
    got = vgg_net.conv3x3_relu(x, w, b).cpu().numpy()
    err, yard = rel_err(got, ref), rel_err(c32, ref)
    print('conv %s -> %d: rel err %.3e  fp32 CPU %.3e  bound %.3e' % (x.shape, Cout, err, yard, 8 * yard))
    assert yard > 0 and err <= 8 * yard


@pytest.mark.parametrize('H,W', [(5, 7), (1, 1), (2, 3)])
def test_pool_pad_never_wins(H, W):
    """all-negative input: a zero pad (or halo) taking part in the last window of an odd extent would win"""
    x = -(np.random.RandomState(H * 10 + W).rand(2, H, W, 64).astype(np.float32) + 0.5)
    got = vgg_net.max_pool_2x2(x).cpu().numpy()
    ref = cpu_pool(x, torch.float64)
    assert got.shape == (2, (H + 1) // 2, (W + 1) // 2, 64)
    assert (got < 0).all() and np.array_equal(got.astype(np.float64), ref)


def test_forward_is_deterministic_and_independent_of_batch(vgg, fixture):
    im = torch.as_tensor(fixture['images_A']).cuda()
    a = vgg.forward(im).cpu().numpy()
    b = vgg.forward(im).cpu().numpy()
    assert np.array_equal(a, b)                                # two calls: bitwise equal
    one = vgg.forward(im[1:2]).cpu().numpy()                   # N = 1 on the max_N = 2 handle
    assert np.array_equal(one, a[1:2])
    both = vgg.forward(im).cpu().numpy()                       # and image 1 of the first pass's buffers is gone
    assert np.array_equal(both, a)


def test_errors_name_the_problem(vgg, weights):
    with pytest.raises(KeyError, match='conv9_9'):
        vgg.load_weights(dict(weights, **{'conv9_9/weights': weights['conv1_1/weights']}))
    bad = dict(weights)
    bad['conv3_2/weights'] = weights['conv3_1/weights']         # [3,3,128,256] where [3,3,256,256] belongs
    with pytest.raises(ValueError, match=r'conv3_2/weights has shape \[3, 3, 128, 256\], expected \[3, 3, 256, 256\]'):
        vgg.load_weights(bad)
    vgg.load_weights(weights)                                  # (the handle stays usable)
    with pytest.raises(ValueError, match='exceeds'):
        vgg.forward(np.zeros((3, 34, 50, 3), np.uint8))
    with pytest.raises(KeyError, match='fc6'):
        vgg.layer('fc6')


def test_load_checkpoint_on_the_device(vgg, fixture, weights, tmp_path):
    prefix = str(tmp_path / 'vgg_net.tfmodel')
    tf_checkpoint.write_checkpoint(prefix, {'vgg_net/' + k: v for k, v in weights.items()})
    want = vgg.forward(fixture['images_A']).cpu().numpy()
    v2 = vgg_net.VGGPool5(max_N=2, max_H=34, max_W=50)
    v2.load_checkpoint(prefix)
    assert np.array_equal(v2.forward(fixture['images_A']).cpu().numpy(), want)
    v2.close()


def test_pool5_feeds_engine_without_host_copy(weights):
    """a 320 x 480 image pair -> (2, 10, 15, 512) on the device -> Engine.forward as image_feat_batch; the logits
    equal those of the same features handed over as a host array"""
    from n2nmn_amd import synth
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import Dims, CLEVR_MODULE_NAMES
    d = Dims(N=2)
    v = vgg_net.VGGPool5(max_N=2)
    v.load_weights(weights)
    im = np.random.RandomState(7).randint(0, 256, size=(2, 320, 480, 3)).astype(np.uint8)
    feat = v.forward(im)
    assert feat.is_cuda and tuple(feat.shape) == (2, d.H, d.W, d.D)
    feat = feat / feat.max()                                   # (still on the device) the scale of trained features
    eng = Engine(d, Assembler(list(CLEVR_MODULE_NAMES)))
    eng.load_weights(synth.make_weights(d, seed=0))
    batch = synth.make_inputs(d, seed=0)
    gt = synth.template_layout_batch(d)
    s_dev, _, ok = eng.forward(dict(batch, image_feat_batch=feat), use_gt_layout=True, gt_layout=gt)
    s_dev = s_dev.cpu().numpy()
    s_host, _, _ = eng.forward(dict(batch, image_feat_batch=feat.cpu().numpy()), use_gt_layout=True, gt_layout=gt)
    s_host = s_host.cpu().numpy()
    assert np.asarray(ok).all() and np.isfinite(s_dev).all() and np.abs(s_dev).max() > 0
    assert np.array_equal(s_dev, s_host)
    v.close()


def test_extract_dataset_pool5(vgg, fixture, tmp_path):
    from PIL import Image
    im = fixture['images_A']
    src, dst = tmp_path / 'images', tmp_path / 'vgg_pool5'
    src.mkdir()
    Image.fromarray(im[0]).save(str(src / 'CLEVR_a.png'))
    rgba = np.concatenate([im[1], np.full(im[1].shape[:2] + (1,), 77, np.uint8)], axis=-1)
    Image.fromarray(rgba, 'RGBA').save(str(src / 'CLEVR_b.png'))
    (src / 'notes.txt').write_text('not an image')
    assert vgg_net.extract_dataset_pool5(str(src), str(dst), vgg=vgg) == 2
    saved = [np.load(str(dst / (name + '.npy'))) for name in ('CLEVR_a', 'CLEVR_b')]
    for a in saved:
        assert a.shape == (1, 2, 2, 512) and a.dtype == np.float32
    assert rel_err(np.concatenate(saved), fixture['pool5_A']) <= TOL
    stamp = {p.name: p.stat().st_mtime_ns for p in dst.iterdir()}
    np.save(str(dst / 'CLEVR_a.npy'), np.zeros(1, np.float32))          # an existing file is kept, whatever it holds
    assert vgg_net.extract_dataset_pool5(str(src), str(dst), vgg=vgg) == 0
    assert np.load(str(dst / 'CLEVR_a.npy')).shape == (1,)
    assert (dst / 'CLEVR_b.npy').stat().st_mtime_ns == stamp['CLEVR_b.npy']
