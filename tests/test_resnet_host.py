"""Host side of the ResNet-152 res5c feature extractor (n2nmn_amd/resnet.py): names and shapes, the extent
arithmetic, batch-norm folding against the unfolded fp64 oracle (tests/resnet_oracle.py), the synthetic weights,
the .npz round trip and the command line.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_oracle as O
from n2nmn_amd import resnet


def test_default_network_has_155_convolutions_with_caffe_names_and_shapes():
    names = resnet.layer_names()
    assert len(names) == 155 and len(set(names)) == 155
    assert names[:5] == ['conv1', 'res2a_branch1', 'res2a_branch2a', 'res2a_branch2b', 'res2a_branch2c']
    assert names[-3:] == ['res5c_branch2a', 'res5c_branch2b', 'res5c_branch2c']
    for n in ('res2c_branch2b', 'res3b1_branch2a', 'res3b7_branch2c', 'res4a_branch1', 'res4b35_branch2c', 'res5a_branch1'):
        assert n in names
    for n in ('res3b_branch2a', 'res3b8_branch2a', 'res4b36_branch2a', 'res2b_branch1', 'res5d_branch2a'):
        assert n not in names
    assert sum(n.endswith('_branch1') for n in names) == 4
    # the oracle spells the same names on its own
    assert [b for st in O.blocks_of((3, 8, 36, 3)) for b in st] == resnet.block_names()
    shapes = dict(resnet.variable_shapes())
    assert len(shapes) == 310
    assert shapes['conv1/weights'] == (7, 7, 3, 64) and shapes['conv1/biases'] == (64,)
    assert shapes['res2a_branch1/weights'] == (1, 1, 64, 256)
    assert shapes['res2a_branch2a/weights'] == (1, 1, 64, 64)
    assert shapes['res2b_branch2a/weights'] == (1, 1, 256, 64)
    assert shapes['res3a_branch1/weights'] == (1, 1, 256, 512)
    assert shapes['res3a_branch2a/weights'] == (1, 1, 256, 128)
    assert shapes['res4b17_branch2b/weights'] == (3, 3, 256, 256)
    assert shapes['res5a_branch2a/weights'] == (1, 1, 1024, 512)
    assert shapes['res5c_branch2b/weights'] == (3, 3, 512, 512)
    assert shapes['res5c_branch2c/weights'] == (1, 1, 512, 2048) and shapes['res5c_branch2c/biases'] == (2048,)
    # 3x3 layers have K = 9 Cin up to 4608, as the tolerance rule of the GPU tests assumes
    assert max(s[0] * s[1] * s[2] for s in shapes.values() if len(s) == 4) == 4608
    assert [n for n, _ in resnet.variable_shapes((1, 1, 1, 1), 32)][-1] == 'res5a_branch2c/biases'
    assert dict(resnet.variable_shapes((1, 1, 1, 1), 32))['res5a_branch2c/weights'] == (1, 1, 256, 1024)


def test_res5c_shape():
    assert resnet.res5c_shape(1, 448, 448) == (1, 14, 14, 2048)
    assert resnet.res5c_shape(8, 224, 224) == (8, 7, 7, 2048)
    assert resnet.res5c_shape(2, 70, 102) == (2, 3, 4, 2048)
    assert resnet.res5c_shape(1, 64, 96, base_width=32) == (1, 2, 3, 1024)


@pytest.mark.parametrize('n', [1, 2, 3, 4, 7, 8, 9, 10, 111, 112, 224])
def test_ceil_mode_pool_extent(n):
    """every parity: the formula, torch's ceil mode, and an explicit clipped-window maximum agree"""
    want = int(np.ceil((n - 3) / 2.0)) + 1 if n >= 3 else 1
    assert resnet.pool_extent(n) == want
    if n >= 3:
        x = -(torch.rand(1, 1, n, n + 1, dtype=torch.float64) + 0.5)          # all negative: a pad of 0 would win
        y = O.pool1(x)
        assert tuple(y.shape[2:]) == (resnet.pool_extent(n), resnet.pool_extent(n + 1))
        clipped = torch.stack([torch.stack([x[0, 0, 2 * i:2 * i + 3, 2 * j:2 * j + 3].max()
                                            for j in range(y.shape[3])]) for i in range(y.shape[2])])
        assert torch.equal(y[0, 0], clipped) and (y < 0).all()


@pytest.mark.parametrize('conv,k,stride,pad,with_bias', [
    ('conv1', 7, 2, 3, True), ('res3a_branch2a', 1, 2, 0, False), ('res2b_branch2b', 3, 1, 1, False)])
def test_folding_equals_unfolded_batchnorm(conv, k, stride, pad, with_bias):
    rs = np.random.RandomState(k)
    cin, cout = (3 if k == 7 else 32), 48
    bn, sc = ('bn_conv1', 'scale_conv1') if conv == 'conv1' else ('bn' + conv[3:], 'scale' + conv[3:])
    raw = {conv + '/weights': rs.randn(k, k, cin, cout).astype(np.float32),
           bn + '/mean': rs.randn(cout).astype(np.float32), bn + '/variance': (0.2 + rs.rand(cout)).astype(np.float32),
           sc + '/gamma': rs.randn(cout).astype(np.float32), sc + '/beta': rs.randn(cout).astype(np.float32)}
    if with_bias:
        raw[conv + '/biases'] = rs.randn(cout).astype(np.float32)
    assert resnet.bn_names(conv) == (bn, sc)
    folded = resnet.fold_batchnorm(raw)
    assert sorted(folded) == [conv + '/biases', conv + '/weights']
    assert folded[conv + '/weights'].dtype == np.float32 and folded[conv + '/weights'].shape == (k, k, cin, cout)
    x = torch.as_tensor(rs.randn(2, cin, 9, 11))
    want = O.conv_bn(x, raw, conv, stride, pad, False, torch.float64)
    got = F.conv2d(x, torch.as_tensor(folded[conv + '/weights']).double().permute(3, 2, 0, 1),
                   torch.as_tensor(folded[conv + '/biases']).double(), stride=stride, padding=pad)
    # the folded pair is rounded to float32 once: 2^-24 per weight and bias
    assert O.rel_err(got.numpy(), want.numpy()) < 4e-7


def test_synthetic_weights_are_reproducible_and_complete():
    blocks = (1, 2, 1, 1)
    a, b = resnet.synthetic_weights(3, blocks, 32), resnet.synthetic_weights(3, blocks, 32)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    c = resnet.synthetic_weights(4, blocks, 32)
    assert not np.array_equal(a['conv1/weights'], c['conv1/weights'])
    assert len(a) == 5 * len(resnet.layer_names(blocks)) and resnet.is_raw(a)
    folded = resnet.fold_batchnorm(a)
    assert [(k, folded[k].shape) for k, _ in resnet.variable_shapes(blocks, 32)] == resnet.variable_shapes(blocks, 32)
    assert (a['bn3b_branch2b/variance'] > 0.89).all()
    # the last layer of a block is damped, the others are not
    assert abs(a['scale2a_branch2c/gamma'].mean() - 0.25) < 0.05 and abs(a['scale2a_branch2a/gamma'].mean() - 1) < 0.1
    # the whole shallow net keeps its scale (fp64 oracle on the raw weights)
    im = np.random.RandomState(0).randint(0, 256, size=(1, 40, 40, 3)).astype(np.uint8)
    acts = O.forward(im, a, blocks)
    assert 0.05 < np.abs(acts['res5a_branch2c']).max() / np.abs(acts['pool1']).max() < 20


def test_npz_round_trip(tmp_path):
    blocks = (1, 1, 1, 1)
    raw = resnet.synthetic_weights(1, blocks, 32)
    folded = resnet.fold_batchnorm(raw)
    np.savez(str(tmp_path / 'raw.npz'), **raw)
    np.savez(str(tmp_path / 'folded.npz'), **folded)
    for name in ('raw.npz', 'folded.npz'):
        got = resnet.load_npz(str(tmp_path / name))
        assert sorted(got) == sorted(folded)
        assert all(np.array_equal(got[k], folded[k]) and got[k].dtype == np.float32 for k in folded)
    flipped = resnet.load_npz(str(tmp_path / 'raw.npz'), bgr_conv1=True)
    assert np.array_equal(flipped['conv1/weights'], folded['conv1/weights'][:, :, ::-1, :])
    assert np.array_equal(flipped['res2a_branch2a/weights'], folded['res2a_branch2a/weights'])


def test_cli_arguments(capsys):
    a = resnet.parse_args(['--weights', 'w.npz', '--images', 'in', '--out', 'resnet_res5c/train2014'])
    assert (a.size, a.batch, a.ext, a.bgr_conv1) == (448, 8, '*.jpg', False)
    assert np.allclose(a.mean, [123.68, 116.779, 103.939])
    a = resnet.parse_args(['--weights', 'w.npz', '--images', 'in', '--out', 'o', '--size', '224', '--bgr-conv1',
                           '--mean', '104', '117', '123', '--batch', '2'])
    assert (a.size, a.batch, a.bgr_conv1, a.mean) == (224, 2, True, [104.0, 117.0, 123.0])
    for bad in (['--images', 'in', '--out', 'o'],                                  # no weights
                ['--weights', 'w.npz', '--images', 'in', '--out', 'o', '--size', '-1'],
                ['--weights', 'w.npz', '--images', 'in', '--out', 'o', '--batch', '0']):
        with pytest.raises(SystemExit):
            resnet.parse_args(bad)
    capsys.readouterr()
