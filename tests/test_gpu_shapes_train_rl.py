"""models_shapes trained from scratch (exp_shapes/train_shapes_scratch.py:204-232: layouts SAMPLED by the decoder,
REINFORCE with an EMA baseline + entropy regulariser + answer loss) on the HIP path against numbers computed by the
REFERENCE'S OWN CODE: tests/golden/shapes_rl_golden.npz = the unmodified models_shapes/*.py with
decoder_sampling=True and the driver's loss / clip / Adam block under the TF1 stand-in
(tests/golden/make_shapes_rl_golden.py).  Uniforms and keep masks are inputs on both sides; every uniform sits in
the middle of the softmax interval of a chosen token, so the sampled layouts are the fixture's by construction.

Two routes are held to the reference, each on its own: the single-pass ShapesTrainer.step_rl (n2nmn_train_sample
samples inside the training forward, <eos> latch in the decoder's token step) and the two-pass
forward_backward(objective=1) on given tokens.

Bars (those of tests/test_gpu_shapes_train.py): tokens and validity identical; log_seq_prob, losses, baseline
1e-4 relative (+1e-6); every clipped gradient 2e-4 * max|g| (+1e-7); weights within lr * 0.2 after one Adam step
and 3 * lr * 0.2 after three."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import float_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'shapes_rl_golden.npz')
CNN = 'neural_module_network/image_feature_cnn/shapes_convnet/'
SEQ2SEQ = 'neural_module_network/layout_generation/'
CASES = ['mixed', 'mixed_nodrop', 'all_invalid', 'one_valid']
GRAD_RTOL = 2e-4
LR = 1e-3
WD = 5e-4
T_DEC = 7
EOS = 4


@pytest.fixture(scope='module')
def fx():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z['meta_json']).decode())


@pytest.fixture(scope='module')
def setup():
    from n2nmn_amd.models_shapes import ShapesTrainer, shapes_engine
    d, batch, gt, w, nv_txt, nv_nmn = FC.shapes_setup()
    with open(os.path.join(HERE, 'golden', 'shapes_golden.json')) as f:
        labels = np.array(json.load(f)['labels'], np.int32)
    b = dict(image_batch=batch['image_batch'], input_seq_batch=batch['text_seq_batch'],
             seq_length_batch=batch['seq_length_batch'], answer_label_batch=labels)
    eng = shapes_engine(nv_txt, N=256, T_decoder=T_DEC)
    tr = ShapesTrainer(eng)
    w32 = {k: np.asarray(v, np.float32) for k, v in w.items()}
    return b, tr, w32


def _reset(tr, w):
    from n2nmn_amd import _lib
    tr.load_weights(w)
    _lib.check(tr._lib.n2nmn_train_reset_optimizer(tr._ctx, tr.engine.stream()))
    tr.iteration = 0
    tr.set_baseline(tr.rl['invalid_expr_loss'])


def _masks(z, case):
    if case == 'mixed_nodrop':
        return False
    return dict(enc0=z['mask_enc0'].astype(np.float32), dec0=z['mask_dec0'].astype(np.float32))


def _clip(g, c=10.0):
    n = float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))
    return g * (c / max(n, c))


def _check_named(z, key, meta, got, tol_of):
    bad = []
    for name, g in got.items():
        g = np.asarray(g, np.float64).reshape(-1)
        if key + '/' + name in z.files and name not in meta:       # stored in full
            want = np.asarray(z[key + '/' + name], np.float64).reshape(-1)
            d = np.max(np.abs(g - want))
            tol = tol_of(np.max(np.abs(want)))
        else:
            d = np.max(np.abs(g[FC.probe_indices(name, g.size)] - z[key + '/' + name]))
            tol = tol_of(meta[name]['absmax'])
        print('%s/%s: max diff %.3e (tol %.3e)' % (key, name, d, tol))
        if not (d <= tol and np.isfinite(g).all()):
            bad.append('%s: max diff %.3e (tol %.3e)' % (name, d, tol))
    assert not bad, '\n'.join(bad)


def _rel(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print('%s: got %s want %s' % (what, got, want))
    assert np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-6), (what, got, want)


def _check_step(tr, z, m, case, losses, tokens, validity):
    """everything the fixture holds about the first iteration, after the step's Adam update"""
    assert np.array_equal(tokens, z[case + '/tokens']), (tokens.T, z[case + '/tokens'].T)
    assert np.array_equal(np.asarray(validity, bool), z[case + '/validity'])
    N = tokens.shape[1]
    lsp = tr.debug_tensor('log_seq_prob', (N,)).cpu().numpy()
    _rel(lsp, z[case + '/log_seq_prob'], 'log_seq_prob')
    _rel(losses.cpu().numpy()[:5], z[case + '/losses'], 'losses')
    _rel(tr.get_baseline(), m['baseline1'], 'baseline')
    scores = tr.scores.cpu().numpy()
    assert np.all(scores[~z[case + '/validity']] == 0.0)
    grads = {k: _clip(v.cpu().numpy()) for k, v in tr.gradients().items()}
    assert set(grads) == set(m['variables'])
    _check_named(z, case + '/grad', m['grad'], grads, lambda a: GRAD_RTOL * a + 1e-7)
    w1 = {k: v.cpu().numpy() for k, v in tr.get_weights().items()}
    _check_named(z, case + '/w1', m['w1'], w1, lambda a: LR * 0.2)


@pytest.mark.parametrize('case', CASES)
def test_shapes_rl_step_matches_reference_code(setup, fx, case):
    """the single-pass step: sample inside the training forward, assemble, module network, backward, Adam"""
    b, tr, w = setup
    z, meta = fx
    m = meta[case]
    _reset(tr, w)
    u = z[case + '/uniforms']
    losses, tokens, validity = tr.step_rl(b, u[0], dropout=_masks(z, case))
    _check_step(tr, z, m, case, losses, tokens, validity)
    for it in (1, 2):
        _, tokens, _ = tr.step_rl(b, u[it], dropout=_masks(z, case))
        assert np.array_equal(tokens, z[case + '/tokens'])
    w3 = {k: v.cpu().numpy() for k, v in tr.get_weights().items()}
    _check_named(z, case + '/w3', m['w3'], w3, lambda a: 3 * LR * 0.2)
    _rel(tr.get_baseline(), m['baseline3'], 'baseline after 3 steps')


@pytest.mark.parametrize('case', CASES)
def test_shapes_rl_two_pass_matches_reference_code(setup, fx, case):
    """the two-pass form on the fixture's tokens: Engine.seq2seq samples (no latch on the device: the tokens in
    front of each row's first <eos> are the fixture's), forward_backward(objective=1) repeats the passes
    teacher-forced on the latched tokens"""
    b, tr, w = setup
    z, meta = fx
    m = meta[case]
    _reset(tr, w)
    u = z[case + '/uniforms']
    want = z[case + '/tokens']
    for it in range(3):
        mult = tr.multipliers(b['input_seq_batch'].shape[0], want.shape[1], T_DEC, _masks(z, case))
        s2s = tr.engine.seq2seq(b['input_seq_batch'], b['seq_length_batch'], T_DEC, sample_uniforms=u[it],
                                dropout=(mult.get('enc0'), mult.get('dec0')))
        raw = s2s['predicted_tokens'].cpu().numpy()
        front = np.cumsum(np.vstack([np.zeros((1, raw.shape[1]), int), (raw == EOS)[:-1]]), axis=0) == 0
        assert np.array_equal(raw[front], want[front])
        scale = tr.forward_backward(b, want, objective=1, dropout=_masks(z, case))
        tr.apply(scale)
        if it == 0:
            _check_step(tr, z, m, case, tr.losses, want, tr.last_validity)
    w3 = {k: v.cpu().numpy() for k, v in tr.get_weights().items()}
    _check_named(z, case + '/w3', m['w3'], w3, lambda a: 3 * LR * 0.2)
    _rel(tr.get_baseline(), m['baseline3'], 'baseline after 3 steps')


def test_shapes_rl_all_invalid_is_weight_decay_only(setup, fx):
    """no layout assembles (the normal case early in training): the program has no node; scores are zero, the
    module and convnet gradient is exactly weight_decay * w on the l2 variables and zero elsewhere, the seq2seq
    variables carry the policy and entropy terms"""
    import torch
    from n2nmn_amd.models_shapes import l2_variables
    b, tr, w = setup
    z, meta = fx
    _reset(tr, w)
    losses, tokens, validity = tr.step_rl(b, z['all_invalid/uniforms'][0], update=False,
                                          dropout=_masks(z, 'all_invalid'))
    torch.cuda.synchronize()                 # (a failed launch would surface here)
    assert not validity.any()
    assert np.all(tr.scores.cpu().numpy() == 0.0)
    l = losses.cpu().numpy()
    assert l[0] == np.float32(tr.rl['invalid_expr_loss'])
    grads = {k: v.cpu().numpy() for k, v in tr.gradients().items()}
    decayed = l2_variables(grads)
    seen = 0
    for k, g in grads.items():
        if k.startswith(SEQ2SEQ):
            continue
        seen += 1
        want = np.float32(WD) * w[k] if k in decayed else np.zeros_like(w[k])
        assert np.array_equal(g, want.astype(np.float32)), k
    assert seen >= 14
    assert any(np.abs(g).max() > 0 for k, g in grads.items() if k.startswith(SEQ2SEQ) and k not in decayed)


def test_shapes_rl_latch_gradient(setup, fx):
    """d token_scores is exactly 0 behind each row's first <eos> and non-zero at it"""
    b, tr, w = setup
    z, meta = fx
    _reset(tr, w)
    _, tokens, _ = tr.step_rl(b, z['mixed/uniforms'][0], update=False, dropout=_masks(z, 'mixed'))
    raw = z['mixed/targets']
    assert (raw != tokens).any()             # the rows with samples behind their <eos>: the latch mattered
    Td, N = tokens.shape
    dsc = tr.debug_tensor('d_token_scores', (Td, N, 16)).cpu().numpy()
    has = (tokens == EOS).any(axis=0)
    first = np.argmax(tokens == EOS, axis=0)
    behind = (np.arange(Td)[:, None] > first[None, :]) & has[None, :]
    assert behind.any() and not has.all()
    assert np.all(dsc[behind] == 0.0)
    rows = np.nonzero(has)[0]
    assert np.all(np.abs(dsc[first[rows], rows, :5]).max(-1) > 0)
    assert np.all(np.abs(dsc[:, ~has, :5]).max(-1) > 0)      # rows without <eos> count every step


def test_shapes_rl_forward_needs_its_sample_pass(setup, fx):
    """n2nmn_train_forward with the sampled-layout objective and no sampling pass in front: N2NMN_EINVAL"""
    from n2nmn_amd import _lib
    b, tr, w = setup
    z, _ = fx
    _reset(tr, w)
    gt = z['mixed/tokens']
    tr.forward_backward(b, gt, objective=1, dropout=False)       # a teacher-forced forward is no sample pass
    io, packed, _ = tr._io(b, gt, 2, False)
    rc = tr._lib.n2nmn_train_forward(tr._ctx, C.byref(io), packed.handle, tr.engine.stream())
    assert rc == -1, rc                      # N2NMN_EINVAL
    assert b'n2nmn_train_sample' in tr._lib.n2nmn_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_shapes_rl_driver_geometry(setup):
    """N = 256 and a short last batch of 100, uniforms from a seeded generator, dropout from the seed stream; then
    one bounded pass of 30 steps: losses finite, the baseline moves from 3 toward avg_sample_loss, validity < 1"""
    b, tr, w = setup
    _reset(tr, w)
    rng = np.random.default_rng(7)

    def big(n):
        idx = rng.integers(0, 12, size=n)
        img = b['image_batch'][idx] + rng.standard_normal(b['image_batch'][idx].shape).astype(np.float32)
        return dict(image_batch=img.astype(np.float32), input_seq_batch=b['input_seq_batch'][:, idx],
                    seq_length_batch=b['seq_length_batch'][idx], answer_label_batch=b['answer_label_batch'][idx])

    for n in (256, 100):
        losses, tokens, validity = tr.step_rl(big(n), rng.random((T_DEC, n), dtype=np.float32))
        assert tokens.shape == (T_DEC, n) and validity.shape == (n,)
        assert np.isfinite(losses.cpu().numpy()[:5]).all(), (n, losses)
    _reset(tr, w)
    bb = big(256)
    avg, val = [], []
    for _ in range(30):
        losses, tokens, validity = tr.step_rl(bb, rng.random((T_DEC, 256), dtype=np.float32))
        l = losses.cpu().numpy()[:5]
        assert np.isfinite(l).all(), l
        avg.append(float(l[0]))
        val.append(float(validity.mean()))
    base = tr.get_baseline()
    print('avg_sample_loss %s\nvalidity %s\nbaseline %.5f' % (avg, val, base))
    assert np.mean(val) < 1.0
    # EMA from 3 with decay 0.99: the baseline has moved toward the losses it saw, and not past them
    lo, hi = min(avg + [3.0]), max(avg + [3.0])
    assert lo <= base <= hi and base != 3.0
    want = 3.0
    for a in avg:
        want += (1 - 0.99) * (a - want)
    assert abs(base - want) <= 1e-4 * abs(want) + 1e-6
