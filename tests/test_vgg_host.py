"""Host side of the VGG-16 pool5 extractor (n2nmn_amd/vgg_net.py): the synthetic-weight helper, the fixture
generator's agreement with the reference code, and checkpoint loading.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from n2nmn_amd import tf_checkpoint, vgg_net

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'vgg_golden.npz')


def test_synthetic_weights_are_deterministic_and_he_scaled():
    a, b = vgg_net.synthetic_weights(0), vgg_net.synthetic_weights(0)
    assert list(a) == [n for n, _ in vgg_net.variable_shapes()] and len(a) == 26
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    c = vgg_net.synthetic_weights(1)
    assert not np.array_equal(a['conv1_1/weights'], c['conv1_1/weights'])
    w = a['conv4_2/weights']
    assert abs(float(w.std()) / np.sqrt(2.0 / (9 * 512)) - 1.0) < 0.01
    assert abs(float(a['conv4_2/biases'].std()) / 0.1 - 1.0) < 0.15


def test_names_and_shapes_are_what_the_reference_code_asks_for():
    """the fixture lists every variable models_clevr/vgg_net.py created under oracle/tf1_stub, in order"""
    asked = json.loads(str(np.load(GOLDEN)['variables']))
    ours = [[n, list(s)] for n, s in vgg_net.variable_shapes()]
    assert ours == asked
    w = vgg_net.synthetic_weights(int(np.load(GOLDEN)['seed']))
    assert [[n, list(w[n].shape)] for n in w] == asked


def test_channel_mean_and_layer_names():
    assert vgg_net.channel_mean.dtype == np.float32
    assert np.array_equal(vgg_net.channel_mean, np.array([123.68, 116.779, 103.939], np.float32))
    assert len(vgg_net.LAYERS) == 18 and vgg_net.LAYERS[0] == 'conv1_1' and vgg_net.LAYERS[-1] == 'pool5'
    assert vgg_net.pool5_shape(1, 320, 480) == (1, 10, 15, 512)
    assert vgg_net.pool5_shape(2, 34, 50) == (2, 2, 2, 512)


@pytest.mark.skipif(not os.path.isdir('/root/reference'), reason='needs the reference checkout')
def test_fixture_regenerates_from_the_reference_code():
    out = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'make_vgg_golden.py'), '--check'],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'max abs difference 0' in out.stdout


def test_checkpoint_round_trip(tmp_path):
    """what a Saver over vgg_pool5(image_batch, 'vgg_net') holds, written by the project's own writer"""
    w = vgg_net.synthetic_weights(3)
    prefix = str(tmp_path / 'vgg_net.tfmodel')
    tf_checkpoint.write_checkpoint(prefix, {'vgg_net/' + k: v for k, v in w.items()})
    got = vgg_net.read_checkpoint_weights(prefix)
    assert list(got) == list(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    other = str(tmp_path / 'other')
    tf_checkpoint.write_checkpoint(other, {'tower/' + k: v for k, v in w.items()})
    assert np.array_equal(vgg_net.read_checkpoint_weights(other, scope='tower')['conv5_3/biases'], w['conv5_3/biases'])
    with pytest.raises(KeyError):
        vgg_net.read_checkpoint_weights(other)                  # no vgg_net/ scope in it
    bad = dict(w)
    bad['conv2_1/weights'] = w['conv2_1/weights'][:, :, :32]
    tf_checkpoint.write_checkpoint(str(tmp_path / 'bad'), {'vgg_net/' + k: v for k, v in bad.items()})
    with pytest.raises(ValueError, match='conv2_1/weights'):
        vgg_net.read_checkpoint_weights(str(tmp_path / 'bad'))
