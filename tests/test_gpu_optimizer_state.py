"""Optimiser state on the GPU: n2nmn_train_get_moments / n2nmn_train_set_moments, Trainer.optimizer_state /
load_optimizer_state for the three trainers, and the drop-in's Saver carrying Adam from a cloning snapshot into
the policy-gradient script's graph.

The training backward uses float atomics, so two runs of one step do not give the same bits and nothing here
compares "3 + 3 steps" with "6 steps".  What is deterministic is compared: the round trip bit for bit, and the
Adam update of a GIVEN gradient against the fp64 formula (oracle.n2nmn_oracle_grad.adam_step) at the 2e-6 of
tests/test_gpu_train.py::test_adam_steps_match_oracle_formula.
"""
import json
import os
import sys

import numpy as np
import pytest

import eval_driver_common as EC
import train_driver_common as TC
from oracle import n2nmn_oracle_grad as G
from n2nmn_amd import synth
from n2nmn_amd import train as T
from n2nmn_amd.spec import CLEVR_MODULE_NAMES, Dims
from util import assert_close, t2n

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLD)
import float_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(CLEVR_MODULE_NAMES)
WD = 5e-6
ADAM_TOL = 2e-6


def _same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _check_keys(st, names):
    keys = T.optimizer_state_keys(list(names))
    assert set(st) == set(keys) and len(st) == len(keys) and list(st)[-4:] == keys[-4:]
    assert int(st[T.ADAM_STEP_KEY]) == 3
    assert st['beta2_power'] == np.float32(float(np.float32(0.999)) ** 4)
    moved = sum(bool(np.any(st[n + '/Adam_1'])) for n in names)
    assert moved >= len(list(names)) // 2, 'three steps leave second moments behind'


# ---- CLEVR --------------------------------------------------------------------------------------------------------------
def _clevr_engine(d, w):
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    eng = Engine(d, Assembler(NAMES))
    eng.load_weights(w)
    return eng


@pytest.fixture(scope='module')
def clevr():
    """trainer A after 3 steps on one batch: its weights, its state, the fp64 moments of the same gradients, and
    the gradient of a fourth, different batch (A has then applied it)"""
    from n2nmn_amd.train import Trainer
    d = Dims(T_decoder=10)                      # the dims of tests/test_gpu_train.py (train_clevr_gt_layout.py:35)
    w = synth.make_weights(d, seed=0)
    a = Trainer(_clevr_engine(d, w), weight_decay=WD)
    batch = synth.make_inputs(d, seed=3)
    gt = synth.template_layout_batch(d, offset=1)
    m = {k: np.zeros(np.shape(x)) for k, x in w.items()}
    v = {k: np.zeros(np.shape(x)) for k, x in w.items()}
    cur = {k: np.asarray(x, np.float64) for k, x in w.items()}
    for step in range(1, 4):
        scale = a.forward_backward(batch, gt, reduce=False)
        g = {k: t2n(t).astype(np.float64) for k, t in a.gradients().items()}
        a.apply(scale)
        cur, m, v = G.adam_step(cur, g, m, v, step)
    w3 = {k: t2n(t) for k, t in a.get_weights().items()}
    state = a.optimizer_state()
    # the fourth gradient comes from other questions, images and layouts, so that it is not the direction the
    # moments already point in
    batch4 = synth.make_inputs(d, seed=29, min_len=1)
    gt4 = synth.template_layout_batch(d, offset=6)
    scale = a.forward_backward(batch4, gt4, reduce=False)
    g4 = a.grads.clone()
    g4_named = {k: t2n(t).astype(np.float64) for k, t in a.gradients().items()}
    a.apply(scale)
    w4_a = {k: t2n(t) for k, t in a.get_weights().items()}
    want4, _, _ = G.adam_step({k: x.astype(np.float64) for k, x in w3.items()}, g4_named, m, v, 4)
    return dict(d=d, a=a, w3=w3, state=state, g4=g4, g4_named=g4_named, w4_a=w4_a, want4=want4, scale=scale)


def test_round_trip_clevr(clevr):
    from n2nmn_amd.train import Trainer
    _check_keys(clevr['state'], clevr['a'].layout)
    b = Trainer(_clevr_engine(clevr['d'], clevr['w3']), weight_decay=WD)
    assert b.iteration == 0 and not any(np.any(x) for k, x in b.optimizer_state().items() if k.endswith('/Adam_1'))
    b.load_optimizer_state(clevr['state'])
    assert b.iteration == 3
    _same_state(b.optimizer_state(), clevr['state'])


def _probe(n, count=64):
    return np.unique(np.linspace(0, n - 1, min(n, count)).astype(np.int64))


def test_resume_continues_adam(clevr):
    """B = fresh engine + trainer with A's weights and state after 3 steps; both get A's fourth gradient.  B's
    update is the fp64 formula at step 4 with the carried moments (2e-6) and equals A's; a trainer that did not
    load the state takes a step-1 update from zero moments and lands more than 0.1 * lr away on most probed
    elements, so the bound tells the two apart."""
    from n2nmn_amd.train import Trainer
    c = clevr
    lr = c['a'].hyper['lr']
    b = Trainer(_clevr_engine(c['d'], c['w3']), weight_decay=WD)
    b.load_optimizer_state(c['state'])
    b.grads.copy_(c['g4'])
    b.apply(c['scale'])
    assert b.iteration == 4
    fresh = Trainer(_clevr_engine(c['d'], c['w3']), weight_decay=WD)
    fresh.grads.copy_(c['g4'])
    fresh.apply(c['scale'])
    got_b = {k: t2n(t) for k, t in b.get_weights().items()}
    got_f = {k: t2n(t) for k, t in fresh.get_weights().items()}
    worst = 0.0
    far = total = 0
    for k, want in c['want4'].items():
        worst = max(worst, assert_close('resumed adam[4] %s' % k, got_b[k], want, ADAM_TOL))
        assert_close('resumed trainer vs the uninterrupted one %s' % k, got_b[k], c['w4_a'][k], ADAM_TOL)
        g = c['g4_named'][k].reshape(-1)
        idx = _probe(g.size)
        idx = idx[g[idx] != 0.0]            # (an element without gradient moves under neither optimiser)
        d = np.abs(got_f[k].reshape(-1).astype(np.float64)[idx] - np.asarray(want).reshape(-1)[idx])
        far += int(np.sum(d > 0.1 * lr))
        total += idx.size
    print('resume: worst |w - formula| %.2e; fresh trainer further than 0.1 lr on %d of %d probes' % (worst, far, total))
    assert total >= 500 and far > total // 2, (far, total)


# ---- models_vqa (padded) ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def vqa_pair():
    from n2nmn_amd.vqa import VQAEngine, VQATrainer
    d, batch, gt = FC.vqa_setup()
    batch = dict(batch, answer_label_batch=FC.vqa_labels(d))
    eng = VQAEngine(d)
    eng.load_weights(FC.vqa_weights(d))
    a = VQATrainer(eng)
    for _ in range(3):
        a.step(batch, gt)                   # dropout multipliers drawn from a's stream
    state = a.optimizer_state()
    eng_b = VQAEngine(d)
    eng_b.load_weights(a.weights_reference_shaped())
    b = VQATrainer(eng_b)
    assert b.dropout_stream.offset == 0
    b.load_optimizer_state(state)
    return d, batch, gt, a, b, state


def test_round_trip_vqa(vqa_pair):
    from n2nmn_amd.vqa import vqa_variable_shapes
    d, batch, gt, a, b, state = vqa_pair
    ref = vqa_variable_shapes(d)
    _check_keys(state, ref)
    assert any(tuple(a.layout[k][2]) != tuple(s) for k, s in ref.items()), 'the engine pads these dimensions'
    for k, s in ref.items():
        assert state[k + '/Adam'].shape == tuple(s) and state[k + '/Adam_1'].shape == tuple(s), k
    assert b.iteration == 3
    _same_state(b.optimizer_state(), state)


def test_dropout_stream_continues(vqa_pair):
    """the stream is counter-based: with the offset restored, B draws the multipliers A draws next"""
    import torch
    d, batch, gt, a, b, state = vqa_pair
    assert int(state[T.DROPOUT_OFFSET_KEY]) == a.dropout_stream.offset > 0
    assert b.dropout_stream.offset == a.dropout_stream.offset
    Tq, N = np.asarray(batch['input_seq_batch']).shape
    ma = a.multipliers(Tq, N, d.T_decoder)
    mb = b.multipliers(Tq, N, d.T_decoder)
    assert list(ma) == list(mb) and len(ma) >= 3
    for k in ma:
        assert torch.equal(ma[k].cpu(), mb[k].cpu()), k
        assert 0.0 < float((ma[k] > 0).float().mean()) < 1.0
    assert b.dropout_stream.offset == a.dropout_stream.offset > int(state[T.DROPOUT_OFFSET_KEY])


# ---- models_shapes (renamed) -----------------------------------------------------------------------------------------------
def test_round_trip_shapes():
    from n2nmn_amd.models_shapes import ShapesTrainer, reference_name, shapes_engine
    d, batch, gt, w, nv_txt, nv_nmn = FC.shapes_setup()
    with open(os.path.join(GOLD, 'shapes_golden.json')) as f:
        labels = np.array(json.load(f)['labels'], np.int32)
    bt = dict(image_batch=batch['image_batch'], input_seq_batch=batch['text_seq_batch'],
              seq_length_batch=batch['seq_length_batch'], answer_label_batch=labels)
    a = ShapesTrainer(shapes_engine(nv_txt, N=256))
    a.load_weights({k: np.asarray(x, np.float32) for k, x in w.items()})
    for _ in range(3):
        a.step(bt, gt)
    state = a.optimizer_state()
    names = [reference_name(k) for k in a.layout]
    assert names != list(a.layout)
    _check_keys(state, names)
    b = ShapesTrainer(shapes_engine(nv_txt, N=256))
    b.load_weights(a.get_weights())
    b.load_optimizer_state(state)
    assert b.iteration == 3 and b.dropout_stream.offset == a.dropout_stream.offset > 0
    _same_state(b.optimizer_state(), state)


# ---- the two-stage recipe through the drop-in runtime --------------------------------------------------------------------------
def _load(name):
    z = np.load(os.path.join(GOLD, name))
    return z, json.loads(bytes(z['meta']))


def _features(ids, d):
    return np.concatenate([EC.feature_of(int(i), d) for i in ids], axis=0)


def test_policy_gradient_script_continues_adam_from_a_cloning_snapshot(tmp_path):
    """train_clevr_gt_layout.py's graph for 3 iterations and its snapshot_saver.save, with the optimiser state
    switched on; then train_clevr_rl_gt_layout.py's graph in a new session and its snapshot_loader.restore
    (:178-179), which runs BEFORE any trainer exists.  The first fine-tuning step is Adam's fourth."""
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.nmn3_model import NMN3Model
    from n2nmn_amd.runtime import tf
    from n2nmn_amd import runtime, runtime_train, tf_checkpoint
    d = TC.train_dims()
    was = runtime.save_optimizer_state(True)
    try:
        # ---- stage 1: behavioural cloning (the statements of tests/test_gpu_train_driver_trace.py) ----
        z, meta = _load('train_driver_trace_gt.npz')
        runtime._MODELS.clear()
        runtime_train._GLOBALS.clear()
        kw = dict(meta['model_kwargs'])
        for k in ('assembler', 'use_gt_layout', 'gt_layout_batch'):
            kw.pop(k)
        sess = tf.Session()
        assembler = Assembler(list(synth.CLEVR_MODULE_NAMES))
        input_seq_batch = tf.placeholder(tf.int32, [None, None])
        seq_length_batch = tf.placeholder(tf.int32, [None])
        image_feat_batch = tf.placeholder(tf.float32, [None, d.H, d.W, d.D])
        expr_validity_batch = tf.placeholder(tf.bool, [None])
        answer_label_batch = tf.placeholder(tf.int32, [None])
        gt_layout_batch = tf.placeholder(tf.int32, [None, None])
        model = NMN3Model(image_feat_batch, input_seq_batch, seq_length_batch, assembler=assembler,
                          use_gt_layout=tf.constant(True, dtype=tf.bool), gt_layout_batch=gt_layout_batch, **kw)
        compiler, scores = model.compiler, model.scores
        ce = tf.nn.sparse_softmax_cross_entropy_with_logits(logits=scores, labels=answer_label_batch)
        avg_sample_loss = tf.reduce_mean(ce)
        total_loss = tf.reduce_mean(-model.log_seq_prob) + avg_sample_loss + meta['weight_decay'] * model.l2_reg
        solver = tf.train.AdamOptimizer()
        gradients = [(tf.clip_by_norm(g, meta['hyper']['max_grad_l2_norm']), v)
                     for g, v in solver.compute_gradients(total_loss)]
        with tf.control_dependencies([solver.apply_gradients(gradients)]):
            train_step = tf.constant(0)
        snapshot_saver = tf.train.Saver(max_to_keep=None)
        sess.run(tf.global_variables_initializer())
        model.load_weights(synth.make_weights(d, seed=3))
        for i in range(3):
            h = sess.partial_run_setup([model.predicted_tokens, model.entropy_reg, scores, avg_sample_loss, train_step],
                                       [input_seq_batch, seq_length_batch, image_feat_batch,
                                        compiler.loom_input_tensor, expr_validity_batch, answer_label_batch,
                                        gt_layout_batch])
            tokens, _ = sess.partial_run(h, (model.predicted_tokens, model.entropy_reg), feed_dict={
                input_seq_batch: z['b%d_input_seq' % i], seq_length_batch: z['b%d_seq_length' % i],
                image_feat_batch: _features(z['b%d_image_ids' % i], d), gt_layout_batch: z['b%d_gt_layout' % i]})
            expr_list, validity = assembler.assemble(tokens)
            feed = compiler.build_feed_dict(expr_list)
            feed[expr_validity_batch] = validity
            feed[answer_label_batch] = z['b%d_labels' % i]
            sess.partial_run(h, (scores, avg_sample_loss, train_step), feed_dict=feed)
        assert train_step._step.trainer.iteration == 3
        snapshot = snapshot_saver.save(sess, str(tmp_path / 'tfmodel' / '00000003'), write_meta_graph=False)
        stored = tf_checkpoint.read_checkpoint(snapshot)
        variables = list(model.variable_shapes())
        assert set(stored) == set(variables) | set(T.optimizer_state_keys(variables))
        w3 = {k: t2n(x) for k, x in model.get_weights().items()}
        del model, train_step, sess

        # ---- stage 2: policy gradient from that snapshot (train_clevr_rl_gt_layout.py) ----
        z, meta = _load('train_driver_trace_rl.npz')
        rl = meta['rl']
        runtime._MODELS.clear()
        runtime_train._GLOBALS.clear()
        kw = dict(meta['model_kwargs'])
        kw.pop('assembler')
        sess = tf.Session()
        assembler = Assembler(list(synth.CLEVR_MODULE_NAMES))
        input_seq_batch = tf.placeholder(tf.int32, [None, None])
        seq_length_batch = tf.placeholder(tf.int32, [None])
        image_feat_batch = tf.placeholder(tf.float32, [None, d.H, d.W, d.D])
        expr_validity_batch = tf.placeholder(tf.bool, [None])
        answer_label_batch = tf.placeholder(tf.int32, [None])
        model = NMN3Model(image_feat_batch, input_seq_batch, seq_length_batch, assembler=assembler, **kw)
        compiler, scores, log_seq_prob = model.compiler, model.scores, model.log_seq_prob
        ce = tf.nn.sparse_softmax_cross_entropy_with_logits(logits=scores, labels=answer_label_batch)
        final = tf.where(expr_validity_batch, ce, tf.ones_like(ce) * rl['invalid_expr_loss'])
        avg_sample_loss = tf.reduce_mean(final)
        baseline = tf.Variable(rl['invalid_expr_loss'], trainable=False, dtype=tf.float32)
        baseline_update_op = tf.assign_add(baseline, (1 - rl['baseline_decay']) * (avg_sample_loss - baseline))
        policy_gradient_loss = tf.reduce_mean(tf.stop_gradient(final - baseline) * log_seq_prob)
        total_loss = tf.add_n([policy_gradient_loss + avg_sample_loss, rl['lambda_entropy'] * model.entropy_reg,
                               meta['weight_decay'] * model.l2_reg])
        solver = tf.train.AdamOptimizer(learning_rate=meta['hyper']['lr'])
        gradients = [(tf.clip_by_norm(g, meta['hyper']['max_grad_l2_norm']), v)
                     for g, v in solver.compute_gradients(total_loss)]
        with tf.control_dependencies([solver.apply_gradients(gradients), baseline_update_op]):
            train_step = tf.constant(0)
        sess.run(tf.global_variables_initializer())
        snapshot_loader = tf.train.Saver([v for v in tf.global_variables() if v != baseline])        # :178
        snapshot_loader.restore(sess, snapshot)                                                       # :179
        assert getattr(model, '_trainer', None) is None, 'no trainer before the first train_step'
        for k, x in model.get_weights().items():
            assert np.array_equal(t2n(x), w3[k]), k
        assert float(sess.run(baseline)) == np.float32(rl['invalid_expr_loss'])
        h = sess.partial_run_setup([model.predicted_tokens, model.entropy_reg, scores, avg_sample_loss, train_step],
                                   [input_seq_batch, seq_length_batch, image_feat_batch, compiler.loom_input_tensor,
                                    expr_validity_batch, answer_label_batch])
        tokens, _ = sess.partial_run(h, (model.predicted_tokens, model.entropy_reg), feed_dict={
            input_seq_batch: z['b0_input_seq'], seq_length_batch: z['b0_seq_length'],
            image_feat_batch: _features(z['b0_image_ids'], d)})
        expr_list, validity = assembler.assemble(tokens)
        feed = compiler.build_feed_dict(expr_list)
        feed[expr_validity_batch] = validity
        feed[answer_label_batch] = z['b0_labels']
        _, loss_val, _ = sess.partial_run(h, (scores, avg_sample_loss, train_step), feed_dict=feed)
    finally:
        runtime.save_optimizer_state(was)
    tr = train_step._step.trainer
    assert tr is model._trainer and tr.iteration == 4
    assert tr.hyper['lr'] == meta['hyper']['lr']
    # baseline: started at invalid_expr_loss (it is not in the snapshot), one EMA update since
    b0, decay = rl['invalid_expr_loss'], rl['baseline_decay']
    assert 'Variable' not in stored and 'baseline' not in stored
    assert abs(float(sess.run(baseline)) - (b0 + (1 - decay) * (float(loss_val) - b0))) <= 1e-5
    # second moments: beta2 * v3 + (1 - beta2) * g^2 with the clipped gradient of this step and the v3 of the
    # snapshot, in fp64 with the float32 betas the C-ABI receives; not the (1 - beta2) * g^2 of a first step
    b1, b2 = float(np.float32(tr.hyper['beta1'])), float(np.float32(tr.hyper['beta2']))
    g = {k: t2n(t).astype(np.float64) for k, t in tr.gradients().items()}
    m3 = {k: stored[k + '/Adam'].astype(np.float64) for k in g}
    v3 = {k: stored[k + '/Adam_1'].astype(np.float64) for k in g}
    zeros = {k: np.zeros_like(x) for k, x in g.items()}
    clip = meta['hyper']['max_grad_l2_norm']
    _, _, v4 = G.adam_step(zeros, g, m3, v3, 4, beta1=b1, beta2=b2, max_grad_l2_norm=clip)
    _, _, v1 = G.adam_step(zeros, g, zeros, zeros, 1, beta1=b1, beta2=b2, max_grad_l2_norm=clip)
    state = tr.optimizer_state()
    worst, probes, one_step = 0.0, 0, 0
    for k in g:
        got = state[k + '/Adam_1'].reshape(-1).astype(np.float64)
        want, first = v4[k].reshape(-1), v1[k].reshape(-1)
        idx = _probe(got.size)
        idx = idx[want[idx] >= 1e-30]       # (float32 holds 2e-6 relative only in its normal range)
        rel = np.abs(got[idx] - want[idx]) / want[idx]
        if idx.size:
            worst = max(worst, float(rel.max()))
        assert np.all(rel <= ADAM_TOL), (k, float(rel.max()))
        probes += idx.size
        one_step += int(np.sum(np.abs(got[idx] - first[idx]) <= ADAM_TOL * np.abs(first[idx])))
    print('two-stage: worst relative |v - formula| %.2e on %d probes; %d of them fit a one-step optimiser'
          % (worst, probes, one_step))
    assert probes >= 500 and one_step < probes // 10


# ---- misuse ------------------------------------------------------------------------------------------------------------------
def test_moment_entry_points_refuse_misuse(clevr):
    import torch
    from n2nmn_amd import _lib
    d = clevr['d']
    eng = _clevr_engine(d, clevr['w3'])          # training never enabled on this one
    L = eng._lib
    buf = torch.zeros(clevr['a'].numel, dtype=torch.float32, device=eng.device)
    for fn, name in ((L.n2nmn_train_get_moments, b'train_get_moments'), (L.n2nmn_train_set_moments, b'train_set_moments')):
        assert fn(eng._ctx, buf.data_ptr(), buf.data_ptr(), eng.stream()) == -1          # N2NMN_EINVAL
        assert name in L.n2nmn_last_error()
        a = clevr['a']
        assert fn(a._ctx, None, None, a.engine.stream()) == -1
        assert name in L.n2nmn_last_error()
        fork = a.engine.fork()
        assert fn(fork._ctx, buf.data_ptr(), buf.data_ptr(), a.engine.stream()) == -1
        assert name in L.n2nmn_last_error()
    with pytest.raises(ValueError):
        _lib.check(L.n2nmn_train_get_moments(eng._ctx, buf.data_ptr(), None, eng.stream()))
    # either pointer alone is fine on a training context
    a = clevr['a']
    assert L.n2nmn_train_get_moments(a._ctx, None, buf.data_ptr(), a.engine.stream()) == 0
    torch.cuda.synchronize()
    assert float(buf.max()) > 0.0


def test_wrong_shaped_slot_names_the_variable(clevr):
    from n2nmn_amd.train import Trainer
    b = Trainer(_clevr_engine(clevr['d'], clevr['w3']), weight_decay=WD)
    name = next(k for k, (_, _, s) in b.layout.items() if len(s) == 2 and s[0] != s[1])
    bad = dict(clevr['state'])
    bad[name + '/Adam'] = bad[name + '/Adam'].T.copy()
    with pytest.raises(ValueError) as e:
        b.load_optimizer_state(bad)
    assert name in str(e.value)
    assert not any(np.any(x) for k, x in b.optimizer_state().items() if k.endswith('/Adam')), 'nothing was loaded'
