"""models_shapes training, host side (no GPU): the variable table of the N2NMN_VARIANT_SHAPES engine against
the reference's models_shapes variables, the weight-decay set against the reference's rule
(models_shapes/nmn3_model.py:104-108), and the fixture of tests/golden/make_shapes_train_golden.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from n2nmn_amd import models_shapes as MS
from oracle import n2nmn_oracle_shapes as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'shapes_train_golden.npz')


def _table():
    d = MS.shapes_dims(num_vocab_txt=14)
    return d, MS.shapes_engine_variable_shapes(d)


def test_shapes_variable_table_is_the_reference_set():
    d, eng = _table()
    mapped = {MS.reference_name(k): tuple(v) for k, v in eng.items()}
    assert len(mapped) == len(eng)
    assert mapped == {k: tuple(v) for k, v in S.variable_shapes(14, 5).items()}
    assert d.variant == MS.VARIANT_SHAPES == 2


def test_shapes_l2_set_is_the_reference_rule():
    _, eng = _table()
    ref = S.variable_shapes(14, 5)
    want = {k for k in ref if 'neural_module_network' in k and k.endswith('weights')}
    # the engine's rule (csrc/capi_train.cpp: names ending in "weights") on its own names, mapped
    got = {MS.reference_name(k) for k in eng if k.endswith('weights')}
    assert got == want == MS.l2_variables(ref)
    assert {S._CNN + 'conv_1/weights', S._CNN + 'conv_2/weights'} <= got
    meta = json.loads(bytes(np.load(GOLDEN)['meta_json']).decode())
    for case in ('drop', 'nodrop'):
        assert set(meta[case]['l2_variables']) == want
        assert set(meta[case]['variables']) == set(ref)
        assert meta[case]['weight_decay'] == 5e-4 and meta[case]['max_grad_l2_norm'] == 10


def test_reference_name_mapping():
    p = 'neural_module_network/layout_execution/'
    assert MS.reference_name(p + 'module_variables/ExistModule/fc_scores/weights') == \
        p + 'AnswerModule/AnswerModule/fc_scores/weights'
    assert MS.reference_name(p + 'module_variables/FindModule/conv_image/biases') == \
        p + 'FindModule/FindModule/conv_image/biases'
    enc = 'neural_module_network/layout_generation/encoder_decoder/encoder/embedding_mat'
    assert MS.reference_name(enc) == enc


@pytest.mark.skipif(not os.path.isdir('/root/reference/models_shapes'),
                    reason='needs a checkout of the reference (models_shapes)')
def test_shapes_train_fixture_regenerates():
    gen = os.path.join(HERE, 'golden', 'make_shapes_train_golden.py')
    p = subprocess.run([sys.executable, gen, '--check'], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
