"""models_shapes trained from scratch, host side (no GPU): the fixture of tests/golden/make_shapes_rl_golden.py is
consistent with the driver's own formulas (exp_shapes/train_shapes_scratch.py:142-161, recomputed here in fp64
numpy from the stored log_seq_prob, validity and cross entropy), its latched tokens assemble to the stored validity
through this project's SHAPES assembler, and the library declares the sampling entry point."""
import json
import os

import numpy as np
import pytest

from n2nmn_amd import _lib
from n2nmn_amd import models_shapes as MS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'shapes_rl_golden.npz')
CASES = ['mixed', 'mixed_nodrop', 'all_invalid', 'one_valid']
EOS = 4


@pytest.fixture(scope='module')
def fx():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z['meta_json']).decode())


def test_library_declares_the_sampling_entry_point():
    assert 'n2nmn_train_sample' in {s[0] for s in _lib.SYMBOLS}
    assert hasattr(_lib.lib(), 'n2nmn_train_sample')


@pytest.mark.parametrize('case', CASES)
def test_fixture_losses_follow_the_driver_formulas(fx, case):
    z, meta = fx
    m = meta[case]
    assert (m['invalid_expr_loss'], m['lambda_entropy'], m['baseline_decay']) == (3, 0.5, 0.99)
    assert (m['weight_decay'], m['max_grad_l2_norm'], m['baseline_before']) == (5e-4, 10, 3.0)
    valid = z[case + '/validity']
    final = np.where(valid, z[case + '/ce'], float(m['invalid_expr_loss']))
    avg = final.mean()
    pg = np.mean((final - m['baseline_before']) * z[case + '/log_seq_prob'])
    entropy = z[case + '/neg_entropy'].mean()
    got_avg, got_pg, l2, total, got_ent = z[case + '/losses']
    assert abs(avg - got_avg) <= 1e-12 and abs(pg - got_pg) <= 1e-12 and abs(entropy - got_ent) <= 1e-12
    assert abs(total - (pg + avg + 0.5 * entropy + 5e-4 * l2)) <= 1e-12
    assert abs(m['baseline1'] - (3.0 + (1 - 0.99) * (avg - 3.0))) <= 1e-12
    lo, hi = sorted((3.0, avg))
    assert lo <= m['baseline1'] <= hi
    # log_seq_prob / neg_entropy stop at each row's first <eos> (probability 1, entropy 0 behind it)
    tok = z[case + '/tokens']
    seen = np.cumsum(tok == EOS, axis=0) > 0
    behind = np.vstack([np.zeros((1, tok.shape[1]), bool), seen[:-1]])
    tp = z[case + '/token_probs']
    assert np.all(tp[behind] == 1.0) and np.all(tp[~behind] < 1.0)
    assert np.allclose(np.log(tp).sum(axis=0), z[case + '/log_seq_prob'], rtol=0, atol=1e-12)
    assert min(m['min_margin']) >= 1e-3


@pytest.mark.parametrize('case', CASES)
def test_fixture_tokens_assemble_to_the_stored_validity(fx, case):
    z, _ = fx
    asm = MS.Assembler(list(MS.SHAPES_MODULE_NAMES))
    tok, raw = z[case + '/tokens'], z[case + '/targets']
    seen = np.cumsum(raw == EOS, axis=0) > 0
    behind = np.vstack([np.zeros((1, raw.shape[1]), bool), seen[:-1]])
    assert np.array_equal(tok, np.where(behind, EOS, raw))
    _, validity = asm.assemble_packed(tok)
    assert np.array_equal(validity, z[case + '/validity'])
    _, raw_validity = asm.assemble_packed(raw)           # (the assembler reads nothing behind the first <eos>)
    assert np.array_equal(raw_validity, validity)


def test_fixture_cases_cover_what_they_claim(fx):
    z, _ = fx
    names = list(MS.SHAPES_MODULE_NAMES)
    tok, valid, raw = z['mixed/tokens'], z['mixed/validity'], z['mixed/targets']
    layouts = {' '.join(names[t] for t in tok[:, n] if t != EOS) for n in np.nonzero(valid)[0]}
    assert {'_Find _Answer', '_Find _Transform _Answer', '_Find _Find _And _Answer'} <= layouts
    assert valid.sum() >= 4 and (~valid).sum() >= 4
    asm = MS.Assembler(names)
    packed, _ = asm.assemble_packed(tok)
    kinds = {packed.status(int(n))[0] for n in np.nonzero(~valid)[0]}
    assert len(kinds) >= 4, kinds             # no <eos>, not enough inputs, stack size != 1, result not ans
    assert (raw != tok).any()                 # samples behind a first <eos>: the latch matters
    assert np.array_equal(z['mixed_nodrop/tokens'], tok)
    assert not z['all_invalid/validity'].any() and z['one_valid/validity'].sum() == 1
    assert z['all_invalid/losses'][0] == 3.0 and np.all(z['all_invalid/scores'] == 0.0)
