"""The table of dimension points (tests/dims_points.py) against the fp64 oracles alone: the inputs the GPU
sweep compares on must reach every operator and every variable, and must not sit on the discontinuities
the gradient comparison has to skip.  No GPU."""
import time

import numpy as np
import pytest

import dims_points as DP
from oracle import n2nmn_oracle as O
from oracle import n2nmn_oracle_grad as G

N_HOST = DP.BATCH_SIZES[0]
ALL_OPS = set(DP.NAMES) - {'<eos>'}


def test_table_is_well_formed():
    names = [p.name for p in DP.POINTS]
    assert len(set(names)) == len(names)
    for p in DP.POINTS:
        d = p.dims
        assert d.variant == 0 and d.num_vocab_nmn == 15 and d.num_layers == 2
        assert d.T_encoder * d.embed_dim_txt + d.T_decoder * d.T_encoder <= 16000
        assert d.N == max(DP.BATCH_SIZES)
        assert (p.refused is None) or p.walker is None
    assert {p.name for p in DP.POINTS if p.forward_only} == {'floor', 'l1152'}


@pytest.mark.parametrize('n', DP.BATCH_SIZES)
@pytest.mark.parametrize('p', DP.POINTS, ids=lambda p: p.name)
def test_layouts_are_valid_and_use_every_operator(p, n):
    toks = DP.layouts(p, n)
    assert toks.shape == (p.dims.T_decoder, n)
    _, validity = O.assemble(DP.NAMES, toks)
    assert validity.all()
    assert DP.operators_used(toks) == ALL_OPS
    b = DP.inputs(p, n)
    lens = b['seq_length_batch']
    assert lens[0] == 1 and lens[1] == p.dims.T_encoder and lens.min() >= 1
    assert (b['input_seq_batch'][np.arange(p.dims.T_encoder)[:, None] >= lens[None, :]] == 0).all()
    bad = DP.invalid_layouts(p, n)
    _, v = O.assemble(DP.NAMES, bad)
    assert not v[list(DP.INVALID_COLUMNS)].any()
    assert v[[i for i in range(n) if i not in DP.INVALID_COLUMNS]].all()


@pytest.mark.parametrize('p', DP.ACCEPTED, ids=lambda p: p.name)
def test_every_variable_gets_a_gradient_and_selections_are_clear(p):
    d = p.dims
    w = DP.weights(p)
    batch = DP.inputs(p, N_HOST)
    toks = DP.layouts(p, N_HOST)
    t0 = time.time()
    ref = O.forward(w, DP.NAMES, batch, d.T_decoder, d.num_choices, np.float64, use_gt_layout=True,
                    gt_layout=toks)
    t1 = time.time()
    # weight decay 0: a non-zero decay would hide a weight matrix the layouts never touch
    _, grads, ex = G.loss_and_grads(w, DP.NAMES, batch, d.T_decoder, d.num_choices, toks, 0.0)
    t2 = time.time()
    assert ref['validity'].all()
    lens = batch['seq_length_batch']
    clear = float((ex['selection_gap'] >= 1e-5).mean())
    print('%s: max |score| %.3e, encoder lengths %d..%d, clear share %.2f, forward %.2f s, gradient %.2f s'
          % (p.name, np.abs(ref['scores']).max(), lens.min(), lens.max(), clear, t1 - t0, t2 - t1))
    assert np.isfinite(ref['scores']).all()
    assert clear >= 0.5
    if p.forward_only:
        return
    dead = [k for k, g in grads.items() if not np.any(g)]
    assert not dead, 'variables with an all-zero oracle gradient: %s' % dead
