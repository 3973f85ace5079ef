"""models_shapes training step (exp_shapes/train_shapes_gt_layout.py:143-163) on the HIP path against numbers
computed by the REFERENCE'S OWN CODE: tests/golden/shapes_train_golden.npz = the unmodified models_shapes/*.py
and the driver's loss / clip / Adam block under the TF1 stand-in (tests/golden/make_shapes_train_golden.py),
with and without dropout (the keep masks are inputs on both sides).

Bar: losses 1e-4 relative, every clipped gradient 2e-4 * max|g| (convnet in full, others as probes),
d image_feat_grid 2e-4 * max, weights after 3 Adam steps within 3 * lr * 0.2."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import float_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shapes_train_golden.npz')
CNN = 'neural_module_network/image_feature_cnn/shapes_convnet/'
GRAD_RTOL = 2e-4
LR = 1e-3


@pytest.fixture(scope='module')
def fx():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z['meta_json']).decode())


@pytest.fixture(scope='module')
def setup():
    from n2nmn_amd.models_shapes import ShapesTrainer, shapes_engine
    d, batch, gt, w, nv_txt, nv_nmn = FC.shapes_setup()
    with open(os.path.join(os.path.dirname(GOLDEN), 'shapes_golden.json')) as f:
        labels = np.array(json.load(f)['labels'], np.int32)
    b = dict(image_batch=batch['image_batch'], input_seq_batch=batch['text_seq_batch'],
             seq_length_batch=batch['seq_length_batch'], answer_label_batch=labels)
    eng = shapes_engine(nv_txt, N=256)
    tr = ShapesTrainer(eng)
    w32 = {k: np.asarray(v, np.float32) for k, v in w.items()}
    return b, gt, tr, w32


def _reset(tr, w):
    from n2nmn_amd import _lib
    tr.load_weights(w)
    _lib.check(tr._lib.n2nmn_train_reset_optimizer(tr._ctx, tr.engine.stream()))
    tr.iteration = 0


def _masks(z, case):
    if case == 'nodrop':
        return False
    return dict(enc0=z[case + '/mask_enc0'].astype(np.float32), dec0=z[case + '/mask_dec0'].astype(np.float32))


def _clip(g, c=10.0):
    n = float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))
    return g * (c / max(n, c))


def _check_named(z, key, meta, got, tol_of):
    bad = []
    for name, g in got.items():
        g = np.asarray(g, np.float64).reshape(-1)
        if name.startswith(CNN):
            want = np.asarray(z[key + '/' + name], np.float64).reshape(-1)
            d = np.max(np.abs(g - want))
            tol = tol_of(np.max(np.abs(want)))
        else:
            m = meta[name]
            d = np.max(np.abs(g[FC.probe_indices(name, g.size)] - z[key + '/' + name]))
            tol = tol_of(m['absmax'])
        if not (d <= tol and np.isfinite(g).all()):
            bad.append('%s: max diff %.3e (tol %.3e)' % (name, d, tol))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('case', ['drop', 'nodrop'])
def test_shapes_training_step_matches_reference_code(setup, fx, case):
    b, gt, tr, w = setup
    z, meta = fx
    m = meta[case]
    _reset(tr, w)
    from n2nmn_amd.models_shapes import reference_name
    assert set(tr.gradients()) == set(m['variables'])
    assert {reference_name(k) for k in tr.engine.variable_names()} == set(m['variables'])
    losses = tr.step(b, gt, dropout=_masks(z, case)).cpu().numpy()[:4]
    want = z[case + '/losses']
    assert np.all(np.abs(losses - want) <= 1e-4 * np.abs(want) + 1e-6), (losses, want)
    # the flat buffer holds d total_loss / d variable; the fixture the driver's clipped gradients
    grads = {k: _clip(v.cpu().numpy()) for k, v in tr.gradients().items()}
    _check_named(z, case + '/grad', m['grad'], grads, lambda a: GRAD_RTOL * a + 1e-7)
    N, H, W, D = 12, 3, 3, 64
    dfeat = tr.debug_tensor('d_image_feat', (N, H, W, D)).cpu().numpy()
    want = z[case + '/d_image_feat_grid']
    assert np.max(np.abs(dfeat - want)) <= GRAD_RTOL * np.max(np.abs(want)) + 1e-9
    w1 = {k: v.cpu().numpy() for k, v in tr.get_weights().items()}
    _check_named(z, case + '/w1', m['w1'], w1, lambda a: LR * 0.2)
    for _ in range(2):
        tr.step(b, gt, dropout=_masks(z, case))
    w3 = {k: v.cpu().numpy() for k, v in tr.get_weights().items()}
    _check_named(z, case + '/w3', m['w3'], w3, lambda a: 3 * LR * 0.2)


def test_shapes_eos_latch(setup, fx):
    """log_seq_prob counts the steps up to and including the first <eos>; later steps get no gradient"""
    b, gt, tr, w = setup
    _reset(tr, w)
    losses = tr.step(b, gt, dropout=False).cpu().numpy()
    Td, N, V = gt.shape[0], gt.shape[1], 5
    sc = tr.debug_tensor('token_scores', (Td, N, V)).cpu().numpy().astype(np.float64)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    logp = np.log(np.take_along_axis(p, gt[..., None].astype(np.int64), -1)[..., 0])       # [Td, N]
    first = np.argmax(gt == V - 1, axis=0)
    assert np.all(gt[first, np.arange(N)] == V - 1)
    upto = np.arange(Td)[:, None] <= first[None, :]
    latched = float(np.mean(-np.sum(np.where(upto, logp, 0.0), axis=0)))
    unlatched = float(np.mean(-np.sum(logp, axis=0)))
    assert abs(losses[1] - latched) <= 1e-4 * abs(latched), (losses[1], latched)
    assert abs(unlatched - latched) > 1e-2 * abs(latched)        # the rows are <eos>-padded: it matters
    dsc = tr.debug_tensor('d_token_scores', (Td, N, 16)).cpu().numpy()
    behind = np.arange(Td)[:, None] > first[None, :]
    assert behind.any()
    assert np.all(dsc[behind] == 0.0)
    assert np.all(np.abs(dsc[first, np.arange(N), :V]).max(-1) > 0)   # the <eos> step itself is counted


def test_shapes_driver_geometry(setup):
    """N = 256 and a smaller last batch, dropout drawn from the seed stream; then 20 steps without dropout on
    a fixed batch lower the total loss"""
    b, gt, tr, w = setup
    _reset(tr, w)
    rng = np.random.default_rng(5)

    def big(n):
        idx = rng.integers(0, 12, size=n)
        img = b['image_batch'][idx] + rng.standard_normal(b['image_batch'][idx].shape).astype(np.float32)
        return dict(image_batch=img.astype(np.float32), input_seq_batch=b['input_seq_batch'][:, idx],
                    seq_length_batch=b['seq_length_batch'][idx],
                    answer_label_batch=b['answer_label_batch'][idx]), np.ascontiguousarray(gt[:, idx])

    for n in (256, 100):
        bb, gg = big(n)
        l = tr.step(bb, gg).cpu().numpy()[:4]
        assert np.isfinite(l).all(), (n, l)
    _reset(tr, w)
    bb, gg = big(256)
    first = float(tr.step(bb, gg, dropout=False).cpu().numpy()[3])
    for _ in range(19):
        last = float(tr.step(bb, gg, dropout=False).cpu().numpy()[3])
    assert np.isfinite(last) and last < first, (first, last)
    names = set(tr.get_weights())
    from oracle import n2nmn_oracle_shapes as S
    assert names == set(S.variable_shapes(14, 5))
