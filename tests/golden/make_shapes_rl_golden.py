#!/usr/bin/env python3
"""Reference-code fixture of the models_shapes policy-gradient step (exp_shapes/train_shapes_scratch.py:204-232):
the reference's unmodified models_shapes/*.py with decoder_sampling=True and the driver's own loss / clip / Adam
block (train_shapes_scratch.py:142-173), run under the eager TF1 / Fold stand-in (oracle/tf1_stub) in float64,
on the 12 dataset questions of float_cases.shapes_setup() with the labels of shapes_golden.json, T_decoder = 7.

The sampled layouts are chosen, not left to chance: uniforms and keep masks are inputs.  For each case the target
token rows below are fed through a stand-in for tf.multinomial that returns the target and records the softmax
interval it owns, step by step; every uniform is the middle of its interval (rounded to float32, the type the GPU
reads); then the step is run again with the stand-in's real inverse-CDF tf.multinomial on those uniforms and
must sample the targets.  Each of the three Adam iterations gets uniforms of its own this way (the driver draws
fresh ones every iteration; the same targets, the moved weights), and every uniform is at least MARGIN away
from both ends of its interval, so fp32 on the GPU cannot flip a token.

Cases: 'mixed' (dropout on: valid rows `_Find _Answer`, `_Find _Transform _Answer`, `_Find _Find _And
_Answer`, ...; invalid rows: no <eos>, not enough inputs, stack size != 1, result not `ans`; rows with
non-<eos> samples behind their first <eos>, which the latch turns into <eos>), 'mixed_nodrop', 'all_invalid',
'one_valid'.

Stored (tests/golden/shapes_rl_golden.npz), per case: uniforms [3, T_dec, N], keep masks, the raw targets, the latched
tokens, validity, log_seq_prob, neg_entropy, the per-row cross entropy, the losses (avg_sample_loss,
policy_gradient_loss, l2_reg, total_loss, entropy_reg), the baseline after 1 and 3 steps, every variable's
CLIPPED gradient (convnet in full as float32, the others as float_cases.probe) and the weights after 1 and 3
Adam steps (float_cases.probe).

    python tests/golden/make_shapes_rl_golden.py [--check]
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_float_golden as G          # noqa: E402  (sets up the stand-in and the reference imports)
import float_cases as FC               # noqa: E402
import make_shapes_train_golden as TG  # noqa: E402
import torch                           # noqa: E402

tf = G.tf
OUT = os.path.join(HERE, 'shapes_rl_golden.npz')
T_DEC = 7
MASK_SEED = 223
STEPS = 3
MARGIN = 1e-3
F, T, A, ANS, E = 0, 1, 2, 3, 4        # exp_shapes/data/vocabulary_layout.txt

# raw samples per row (what tf.multinomial returns; the latch overwrites what follows a row's first <eos>)
VALID_ROWS = [
    [F, ANS, E, E, E, E, E],           # _Find _Answer
    [F, T, ANS, E, E, E, E],           # _Find _Transform _Answer
    [F, F, A, ANS, E, E, E],           # _Find _Find _And _Answer
    [F, ANS, E, F, T, A, ANS],         # _Find _Answer, samples behind the <eos>
    [F, T, T, ANS, E, T, F],           # _Find _Transform _Transform _Answer, samples behind the <eos>
    [F, F, A, T, ANS, E, E],           # _Find _Find _And _Transform _Answer
]
INVALID_ROWS = [
    [F, F, F, T, F, A, ANS],           # no <eos>
    [A, F, ANS, E, E, E, E],           # not enough inputs for _And
    [F, F, ANS, E, E, E, E],           # final stack size 2
    [F, T, E, E, E, E, E],             # result is att, not ans
    [T, E, F, ANS, E, F, F],           # not enough inputs for _Transform; samples behind the <eos>
    [E, F, ANS, E, E, E, E],           # empty layout (stack size 0); a valid layout behind the <eos>
    [F, ANS, F, ANS, A, T, F],         # no <eos>
    [F, F, F, A, E, ANS, E],           # final stack size 2; samples behind the <eos>
]


def targets(case):
    """[T_DEC, 12] raw target samples of a case"""
    v, i = VALID_ROWS, INVALID_ROWS
    if case in ('mixed', 'mixed_nodrop'):
        rows = [v[0], i[0], v[1], i[1], v[2], i[2], v[3], i[3], v[4], i[4], v[5], i[5]]
    elif case == 'all_invalid':
        rows = [i[k % len(i)] for k in range(12)]
    else:                                  # one_valid: row 7 alone assembles
        rows = [i[(k + 3) % len(i)] for k in range(12)]
        rows[7] = v[4]
    return np.array(rows, np.int32).T.copy()


def latch(tok):
    seen = np.cumsum(tok == E, axis=0) > 0
    behind = np.vstack([np.zeros((1, tok.shape[1]), bool), seen[:-1]])
    out = tok.copy()
    out[behind] = E
    return out


class _TF:
    """the stand-in with tf.Variable handing back the baseline the previous iteration left (the driver's
    baseline lives across iterations; every iteration here builds a fresh graph)"""

    def __init__(self, baseline):
        self._baseline = baseline

    def __getattr__(self, k):
        return getattr(tf, k)

    def Variable(self, initial_value, **kw):
        v = tf.Variable(initial_value, **kw)
        if self._baseline is not None:
            v.fill_(self._baseline)
        return v


def one_step(w, batch, lab, d, nv_txt, nv_nmn, mk, gt, sampler, uniforms, prev_solver, baseline):
    """build the sampling graph on weights w and run the driver's loss block.  sampler: replacement for
    tf.multinomial (the interval-recording pass) or None (the stand-in's own, on `uniforms`)"""
    from models_shapes.nmn3_assembler import Assembler
    from models_shapes.nmn3_model import NMN3ModelAtt
    N = batch['image_batch'].shape[0]
    G.fresh_graph(w, N, requires_grad=True)
    drop = mk is not None
    if drop:
        it = iter([mk['enc0'][t] for t in range(d['T_encoder'])] + [mk['dec0'][t] for t in range(T_DEC)])

        def next_mask(shape, keep_prob):
            m = next(it)
            assert tuple(shape) == m.shape and keep_prob == 0.5, (shape, m.shape, keep_prob)
            return m
        tf.config.dropout_masks = next_mask
    real = tf.multinomial
    if sampler is not None:
        tf.multinomial = sampler
    else:
        rows = iter(uniforms)
        tf.config.multinomial_uniforms = lambda nrows: next(rows)
    asm = Assembler(os.path.join(G.REF, 'exp_shapes/data/vocabulary_layout.txt'))
    try:
        model = NMN3ModelAtt(G.T64(batch['image_batch']), torch.as_tensor(batch['text_seq_batch']),
                             torch.as_tensor(batch['seq_length_batch']), T_decoder=T_DEC,
                             num_vocab_txt=nv_txt, embed_dim_txt=d['embed_dim_txt'], num_vocab_nmn=nv_nmn,
                             embed_dim_nmn=d['embed_dim_nmn'], lstm_dim=d['lstm_dim'], num_layers=2,
                             EOS_idx=asm.EOS_idx, encoder_dropout=drop, decoder_dropout=drop,
                             decoder_sampling=True, num_choices=d['num_choices'])
    finally:
        tf.multinomial = real
        tf.config.multinomial_uniforms = None
    if drop:
        assert next(it, None) is None, 'not every dropout mask was consumed'
        tf.config.dropout_masks = None
    if sampler is not None:
        return None, model, None, None
    tokens = G.n(model.predicted_tokens).astype(np.int32)
    exprs, validity = asm.assemble(tokens)
    validity = np.asarray(validity, bool)
    # under TF-Fold td.Compiler.create makes every module's variables; the eager stand-in makes them when a
    # module first runs, so one evaluation on the dataset's own layouts (every module occurs) goes first
    warm, ok = asm.assemble(gt)
    assert np.all(ok)
    tf.Session().run(model.scores, feed_dict=model.compiler.build_feed_dict(warm))
    scores = tf.Session().run(model.scores, feed_dict=model.compiler.build_feed_dict(exprs))
    l2_reg = tf.add_n([tf.nn.l2_loss(v) for v in tf.trainable_variables()
                       if 'neural_module_network' in v.op.name and v.op.name.endswith('weights')])
    proxy = types.SimpleNamespace(compiler=model.compiler, scores=scores, log_seq_prob=model.log_seq_prob,
                                  l2_reg=l2_reg, entropy_reg=model.entropy_reg)
    env = G.exec_loss_block('exp_shapes/train_shapes_scratch.py', dict(
        tf=_TF(baseline), nmn3_model=proxy, vqa_label_batch=torch.as_tensor(lab),
        expr_validity_batch=torch.as_tensor(validity)), first='compiler = nmn3_model.compiler')
    if prev_solver is not None:                      # one AdamOptimizer across the iterations
        env['solver'].t, env['solver'].m, env['solver'].v = prev_solver.t, prev_solver.m, prev_solver.v
    return env, model, tokens, validity


def intervals(w, batch, lab, d, nv_txt, nv_nmn, mk, gt, tgt):
    """(lo, hi) [T_DEC, N]: the share of [0, 1) in which the stand-in's tf.multinomial returns the target"""
    lo, hi = [], []

    def sampler(logits, num_samples):
        t = len(lo)
        p = torch.softmax(torch.as_tensor(logits), dim=1)
        cdf = torch.cumsum(p, dim=1)
        cdf = (cdf / cdf[:, -1:]).detach().numpy()
        k = tgt[t]
        rows = np.arange(len(k))
        hi.append(np.where(k == cdf.shape[1] - 1, 1.0, cdf[rows, k]))
        lo.append(np.where(k > 0, cdf[rows, np.maximum(k - 1, 0)], 0.0))
        return torch.as_tensor(k.astype(np.int64)).reshape(-1, 1)

    one_step(w, batch, lab, d, nv_txt, nv_nmn, mk, gt, sampler, None, None, None)
    assert len(lo) == T_DEC
    return np.array(lo), np.array(hi)


def named_out(out, key, named, full_cnn):
    """float_cases.probe of every tensor; the convnet's in full (float32) where full_cnn"""
    meta = {}
    for k, v in named.items():
        if full_cnn and k.startswith(TG.CNN):
            out[key + '/' + k] = G.n(v).astype(np.float32)
        else:
            meta.update(G.probes(out, key, {k: v}))
    return meta


def generate():
    d, batch, gt, w0, nv_txt, nv_nmn = FC.shapes_setup()
    lab = TG.labels()
    N = batch['image_batch'].shape[0]
    rng = np.random.default_rng(MASK_SEED)
    mk_drop = dict(enc0=(rng.random((d['T_encoder'], N, d['lstm_dim'])) < 0.5).astype(np.float32),
                   dec0=(rng.random((T_DEC, N, d['lstm_dim'])) < 0.5).astype(np.float32))
    out, meta = {}, {}
    out['mask_enc0'] = mk_drop['enc0'].astype(bool)      # one set of keep masks for every case with dropout
    out['mask_dec0'] = mk_drop['dec0'].astype(bool)
    for case in ('mixed', 'mixed_nodrop', 'all_invalid', 'one_valid'):
        mk = None if case == 'mixed_nodrop' else mk_drop
        tgt = targets(case)
        want_tokens = latch(tgt)
        out[case + '/targets'] = tgt
        m = dict(min_margin=[])
        w, solver, baseline = dict(w0), None, None
        uniforms = []
        for it in range(STEPS):
            # this iteration's uniforms (the driver draws fresh ones every iteration): the middle of the
            # interval each target owns on this iteration's weights
            lo, hi = intervals(w, batch, lab, d, nv_txt, nv_nmn, mk, gt, tgt)
            u = (0.5 * (lo + hi)).astype(np.float32)
            uniforms.append(u)
            u64 = u.astype(np.float64)
            margin = float(np.min(np.minimum(u64 - lo, hi - u64)))
            assert margin >= MARGIN, '%s iteration %d: a uniform is %.2e from its interval edge' % (case, it, margin)
            m['min_margin'].append(margin)
            env, model, tokens, validity = one_step(w, batch, lab, d, nv_txt, nv_nmn, mk, gt, None, u64,
                                                    solver, baseline)
            assert np.array_equal(tokens, want_tokens), (case, it, tokens.T, want_tokens.T)
            if it == 0:
                out[case + '/tokens'] = tokens
                out[case + '/validity'] = validity
                out[case + '/log_seq_prob'] = G.n(model.log_seq_prob)
                out[case + '/neg_entropy'] = G.n(model.neg_entropy)
                out[case + '/token_probs'] = G.n(model.token_probs)
                out[case + '/scores'] = G.n(env['scores'])
                out[case + '/ce'] = G.n(env['softmax_loss_per_sample'])
                out[case + '/losses'] = np.array([float(env[k].detach()) for k in (
                    'avg_sample_loss', 'policy_gradient_loss')] + [float(env['nmn3_model'].l2_reg.detach()),
                                                                   float(env['total_loss'].detach()),
                                                                   float(env['nmn3_model'].entropy_reg.detach())])
                m.update(weight_decay=env['weight_decay'], max_grad_l2_norm=env['max_grad_l2_norm'],
                         invalid_expr_loss=env['invalid_expr_loss'], lambda_entropy=env['lambda_entropy'],
                         baseline_decay=env['baseline_decay'], baseline_before=float(env['baseline']),
                         variables=sorted(v.op.name for v in tf.trainable_variables()),
                         l2_variables=sorted(v.op.name for v in tf.trainable_variables()
                                             if 'neural_module_network' in v.op.name and
                                             v.op.name.endswith('weights')))
                m['grad'] = named_out(out, case + '/grad', {v.op.name: g for g, v in env['gradients']}, True)
            env['solver_op'].run()
            env['baseline_update_op'].run()
            solver, baseline = env['solver'], float(env['baseline'])
            w = {v.op.name: G.n(v).copy() for v in tf.trainable_variables()}
            if it + 1 in (1, STEPS):
                m['w%d' % (it + 1)] = named_out(out, case + '/w%d' % (it + 1), w, False)
                m['baseline%d' % (it + 1)] = baseline
        out[case + '/uniforms'] = np.array(uniforms)      # [STEPS, T_DEC, N]
        meta[case] = m
        print('%s: validity %s losses %s margins %s' % (case, out[case + '/validity'].astype(int),
                                                        out[case + '/losses'], m['min_margin']), flush=True)
    out['meta_json'] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    return out


def main():
    out = generate()
    if '--check' in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), 'fixture keys changed'
        worst = 0.0
        for k in out:
            if k == 'meta_json':
                continue
            a, b = np.asarray(old[k], np.float64), np.asarray(out[k], np.float64)
            worst = max(worst, float(np.max(np.abs(a - b))) if a.size else 0.0)
        print('committed fixture vs regenerated: max |diff| = %.3e' % worst)
        assert worst <= 1e-12
        return
    np.savez_compressed(OUT, **out)
    print('wrote %s (%.1f KB)' % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == '__main__':
    main()
