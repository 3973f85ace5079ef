#!/usr/bin/env python3
"""Reference-code fixture of the models_shapes training step (exp_shapes/train_shapes_gt_layout.py:143-163):
the reference's unmodified models_shapes/*.py (NMN3ModelAtt = shapes_convnet + the layout generator with its
<eos> latch + the modules) and the driver's own loss / clip / Adam block, run under the eager TF1 / Fold
stand-in (oracle/tf1_stub) in float64, on the 12 dataset questions of float_cases.shapes_setup() with the
labels of shapes_golden.json.

Two cases: 'drop' (encoder_dropout = decoder_dropout = True as the driver sets them, train_shapes_gt_layout.py:
31-32; TF draws the keep masks from its RNG, here they are inputs handed to the graph through
tf.config.dropout_masks in the order it asks for them: T_enc encoder steps, then T_dec decoder steps) and
'nodrop'.  decoder_sampling is off: with use_gt_layout the decoder's tokens are the ground truth either way.

Stored (tests/golden/shapes_train_golden.npz), per case: the keep masks, answer logits, token_probs,
log_seq_prob, the four loss terms, every variable's CLIPPED gradient (convnet variables in full as float32, the others as
float_cases.probe), d image_feat_grid, and the weights after 1 and after 3 Adam steps on the same batch
(convnet in full as float32, others as probes).

    python tests/golden/make_shapes_train_golden.py [--check]
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
import torch                           # noqa: E402

tf = G.tf
OUT = os.path.join(HERE, 'shapes_train_golden.npz')
CNN = 'neural_module_network/image_feature_cnn/shapes_convnet/'
MASK_SEED = 211
STEPS = 3


def labels():
    with open(os.path.join(HERE, 'shapes_golden.json')) as f:
        return np.array(json.load(f)['labels'], np.int32)


def masks(d, N):
    rng = np.random.default_rng(MASK_SEED)
    return dict(enc0=(rng.random((d['T_encoder'], N, d['lstm_dim'])) < 0.5).astype(np.float32),
                dec0=(rng.random((d['T_decoder'], N, d['lstm_dim'])) < 0.5).astype(np.float32))


def one_step(w, batch, gt, lab, d, nv_txt, nv_nmn, mk, prev_solver):
    """build the graph on weights w, run the driver's loss block; returns (env, model, scores, d feat)"""
    from models_shapes.nmn3_assembler import Assembler
    from models_shapes.nmn3_model import NMN3ModelAtt
    N = batch['image_batch'].shape[0]
    G.fresh_graph(w, N, requires_grad=True)
    drop = mk is not None
    if drop:
        it = iter([mk['enc0'][t] for t in range(d['T_encoder'])] + [mk['dec0'][t] for t in range(d['T_decoder'])])

        def next_mask(shape, keep_prob):
            m = next(it)
            assert tuple(shape) == m.shape and keep_prob == 0.5, (shape, m.shape, keep_prob)
            return m
        tf.config.dropout_masks = next_mask
    asm = Assembler(os.path.join(G.REF, 'exp_shapes/data/vocabulary_layout.txt'))
    model = NMN3ModelAtt(G.T64(batch['image_batch']), torch.as_tensor(batch['text_seq_batch']),
                         torch.as_tensor(batch['seq_length_batch']), T_decoder=d['T_decoder'],
                         num_vocab_txt=nv_txt, embed_dim_txt=d['embed_dim_txt'], num_vocab_nmn=nv_nmn,
                         embed_dim_nmn=d['embed_dim_nmn'], lstm_dim=d['lstm_dim'], num_layers=2,
                         EOS_idx=asm.EOS_idx, encoder_dropout=drop, decoder_dropout=drop,
                         decoder_sampling=False, num_choices=d['num_choices'],
                         use_gt_layout=torch.tensor(True), gt_layout_batch=torch.as_tensor(gt))
    if drop:
        assert next(it, None) is None, 'not every dropout mask was consumed'
        tf.config.dropout_masks = None
    exprs, validity = asm.assemble(G.n(model.predicted_tokens))
    assert np.all(validity)
    dfeat = {}
    model.image_feat_grid.register_hook(lambda g: dfeat.setdefault('g', g.detach().clone()))
    scores = tf.Session().run(model.scores, feed_dict=model.compiler.build_feed_dict(exprs))
    # l2_reg by the model's own rule (models_shapes/nmn3_model.py:104-108), evaluated once every variable
    # exists: under TF-Fold the module variables are created by td.Compiler.create, in front of that line; the
    # eager stand-in creates them when the compiled block first runs, after it (its model.l2_reg then misses
    # the modules' weights)
    l2_reg = tf.add_n([tf.nn.l2_loss(v) for v in tf.trainable_variables()
                       if 'neural_module_network' in v.op.name and v.op.name.endswith('weights')])
    proxy = types.SimpleNamespace(compiler=model.compiler, scores=scores, log_seq_prob=model.log_seq_prob,
                                  l2_reg=l2_reg)
    env = G.exec_loss_block('exp_shapes/train_shapes_gt_layout.py', dict(
        tf=tf, nmn3_model=proxy, vqa_label_batch=torch.as_tensor(lab)), first='compiler = nmn3_model.compiler')
    if prev_solver is not None:                      # one AdamOptimizer across the iterations
        env['solver'].t, env['solver'].m, env['solver'].v = prev_solver.t, prev_solver.m, prev_solver.v
    return env, model, scores, dfeat['g']


def weights_out(out, key, named):
    meta = {}
    for k, v in named.items():
        if k.startswith(CNN):                        # (float32: the fixture stays small)
            out[key + '/' + k] = G.n(v).astype(np.float32)
        else:
            meta.update(G.probes(out, key, {k: v}))
    return meta


def generate():
    d, batch, gt, w0, nv_txt, nv_nmn = FC.shapes_setup()
    lab = labels()
    N = batch['image_batch'].shape[0]
    out, meta = {}, {}
    for case in ('drop', 'nodrop'):
        mk = masks(d, N) if case == 'drop' else None
        if mk is not None:
            out[case + '/mask_enc0'] = mk['enc0'].astype(bool)
            out[case + '/mask_dec0'] = mk['dec0'].astype(bool)
        m = {}
        w, solver = dict(w0), None
        for it in range(STEPS):
            env, model, scores, dfeat = one_step(w, batch, gt, lab, d, nv_txt, nv_nmn, mk, solver)
            if it == 0:
                out[case + '/scores'] = G.n(scores)
                out[case + '/token_probs'] = G.n(model.token_probs)
                out[case + '/log_seq_prob'] = G.n(model.log_seq_prob)
                out[case + '/d_image_feat_grid'] = G.n(dfeat)
                out[case + '/losses'] = np.array([float(env[k].detach()) for k in (
                    'avg_sample_loss', 'seq_likelihood_loss')] + [float(env['nmn3_model'].l2_reg.detach()),
                                                                  float(env['total_loss'].detach())])
                m.update(weight_decay=env['weight_decay'], max_grad_l2_norm=env['max_grad_l2_norm'],
                         fold_batches=model.compiler.batch_sizes,
                         variables=sorted(v.op.name for v in tf.trainable_variables()),
                         l2_variables=sorted(v.op.name for v in tf.trainable_variables()
                                             if 'neural_module_network' in v.op.name and
                                             v.op.name.endswith('weights')))
                m['grad'] = weights_out(out, case + '/grad', {v.op.name: g for g, v in env['gradients']})
            env['solver_op'].run()
            solver = env['solver']
            w = {v.op.name: G.n(v).copy() for v in tf.trainable_variables()}
            if it + 1 in (1, STEPS):
                m['w%d' % (it + 1)] = weights_out(out, case + '/w%d' % (it + 1), w)
        meta[case] = m
        print('%s: losses %s' % (case, out[case + '/losses']), flush=True)
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
