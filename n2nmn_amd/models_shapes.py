"""Python face of the reference's `models_shapes` package for exp_shapes/eval_shapes.py (BASELINE.json
configs[0], the reference's own CPU-runnable plumbing case): the names, constructor arguments and attributes
that script uses (exp_shapes/eval_shapes.py:23-24,73,122-132,138-175), over the HIP engine.

    from models_shapes.nmn3_assembler import Assembler  -> n2nmn_amd.models_shapes.Assembler
    from models_shapes.nmn3_model import NMN3ModelAtt   -> n2nmn_amd.models_shapes.NMN3ModelAtt

    NMN3ModelAtt(image_batch, text_seq_batch, seq_length_batch, T_decoder, num_vocab_txt, embed_dim_txt,
                 num_vocab_nmn, embed_dim_nmn, lstm_dim, num_layers, EOS_idx, encoder_dropout,
                 decoder_dropout, decoder_sampling, num_choices, use_gt_layout=None, gt_layout_batch=None,
                 scope='neural_module_network', reuse=None)             (models_shapes/nmn3_model.py:15-21)
    .predicted_tokens .word_vecs .atts       phase 1 (:29-50)        .compiler .scores      phase 2 (:52-100)

What models_shapes is made of, and where it runs here:
  * shapes_convnet (models_shapes/shapes_convnet.py:8-17): a 10x10 stride-10 VALID convolution + ReLU and a
    1x1 convolution + ReLU = two GEMMs over im2col rows -> n2nmn_fc_forward (the reshape / permute that
    builds the rows is data movement, done on the torch tensor);
  * the layout generator (models_shapes/nmn3_netgen_att.py): the CLEVR encoder / decoder kernels at lstm_dim
    256 WITHOUT a validity automaton (all-zero tables: every token valid at every step) and with the
    reference's <eos> latch (:215-222: every token behind the first <eos> is <eos>) applied to the fetched
    tokens -- the tokens in front of it, which are all the assembler reads, do not depend on it;
  * the modules (models_shapes/nmn3_modules.py:27-144): Find at map_dim 500, Transform with a 3x3 kernel, And,
    Answer = fc([min, mean, max]) = the CLEVR operators' kernels (Answer has ExistModule's arithmetic).
token_probs / neg_entropy / log_seq_prob of models_shapes follow the latch too (probability 1, entropy 0 behind
the <eos>) and are not offered by this inference face.

Training (exp_shapes/train_shapes_gt_layout.py:143-163) is `ShapesTrainer`: an engine of the model variant
N2NMN_VARIANT_SHAPES (include/n2nmn.h), whose training step runs shapes_convnet forward and backward, the <eos>
latch of the teacher-forced loss and layer-0 LSTM dropout on the GPU.  A trained model is evaluated through
this face: NMN3ModelAtt.load_weights(trainer.get_weights()).

Training from scratch (exp_shapes/train_shapes_scratch.py:204-232) is `ShapesTrainer.step_rl`: the layouts are
sampled inside the training forward, once (n2nmn_train_sample: convnet, encoder, decoder in sampling mode with the
activations kept and the <eos> latch in the decoder's token step -- token <eos>, probability 1, entropy 0, <eos>
embedding fed on, behind a row's first <eos>), fetched and assembled on the host, and the step continues with the
module network and the policy-gradient loss (objective N2NMN_OBJ_POLICY_GRADIENT_SAMPLED).  Most sampled layouts
do not assemble early in training; a batch with no valid layout has an empty program, zero scores and, for the
modules and the convnet, the weight-decay gradient alone.  `forward_backward(..., objective=1)` is the two-pass
form on tokens of the caller's choosing.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .engine import Engine, _torch
from .nmn3_assembler import Assembler as _Assembler
from .nmn3_model import Compiler
from .runtime import Fetch, Phase1Inputs, register_model, resolve, to_numpy
from .spec import Dims, variable_shapes
from .train import DROPOUT_FIELDS, Trainer

SHAPES_MODULE_NAMES = ('_Find', '_Transform', '_And', '_Answer', '<eos>')   # exp_shapes/data/vocabulary_layout.txt
# module -> C-ABI operator; _Answer = fc([min, mean, max]) is ExistModule's arithmetic (nmn3_modules.py:122-144)
SHAPES_OP_CODE = {'_Find': 1, '_Transform': 4, '_And': 5, '_Filter': 2, '_Answer': 7}
SHAPES_INPUT_NUM = {'_Find': 0, '_Transform': 1, '_And': 2, '_Filter': 1, '_Answer': 1}   # nmn3_assembler.py:9-18
SHAPES_OUTPUT_TYPE = {'_Find': 'att', '_Transform': 'att', '_And': 'att', '_Filter': 'att', '_Answer': 'ans'}
_P = 'neural_module_network/'
_CNN = _P + 'image_feature_cnn/shapes_convnet/'
_MOD = _P + 'layout_execution/'


class Assembler(_Assembler):
    """models_shapes/nmn3_assembler.py: Assembler(module_vocab_file)"""

    def __init__(self, module_vocab_file):
        super().__init__(module_vocab_file, op_code=SHAPES_OP_CODE, input_num=SHAPES_INPUT_NUM,
                         output_type=SHAPES_OUTPUT_TYPE)


class NMN3ModelAtt:
    def __init__(self, image_batch, text_seq_batch, seq_length_batch, T_decoder, num_vocab_txt, embed_dim_txt,
                 num_vocab_nmn, embed_dim_nmn, lstm_dim, num_layers, EOS_idx, encoder_dropout,
                 decoder_dropout, decoder_sampling, num_choices, use_gt_layout=None, gt_layout_batch=None,
                 scope='neural_module_network', reuse=None, engine: Engine = None, device: int = 0,
                 max_batch: int = 256, T_encoder: int = 15, map_dim: int = 500, feat_dim: int = 64,
                 hidden_dim: int = 64, kernel_size: int = 3, beam_size: int = 1):
        if encoder_dropout or decoder_dropout or decoder_sampling:
            raise NotImplementedError('the inference face takes no dropout / sampling (exp_shapes/eval_shapes.py:33-35)')
        names = list(SHAPES_MODULE_NAMES)
        if num_vocab_nmn != len(names) or EOS_idx != names.index('<eos>'):
            raise ValueError('models_shapes layout vocabulary is %r' % (names,))
        shp = getattr(image_batch, 'shape', None)
        if shp is None or len(shp) != 4 or any(s is None for s in shp[1:]):
            raise ValueError('image_batch needs a static [N, H_im, W_im, 3] shape')
        self.H_im, self.W_im, self.C_im = int(shp[1]), int(shp[2]), int(shp[3])
        self.stride = 10                                       # shapes_convnet: kernel 10, stride 10, VALID
        if self.H_im % self.stride or self.W_im % self.stride:
            raise ValueError('image size must be a multiple of the 10x10 stride-10 kernel')
        self.assembler = _Assembler(names, op_code=SHAPES_OP_CODE, input_num=SHAPES_INPUT_NUM,
                                    output_type=SHAPES_OUTPUT_TYPE)
        if engine is None:
            dims = Dims(H=self.H_im // self.stride, W=self.W_im // self.stride, D=feat_dim, map_dim=map_dim,
                        embed_dim_txt=embed_dim_txt, embed_dim_nmn=embed_dim_nmn, lstm_dim=lstm_dim,
                        num_layers=num_layers, num_vocab_txt=num_vocab_txt, num_vocab_nmn=num_vocab_nmn,
                        num_choices=num_choices, T_encoder=T_encoder, T_decoder=T_decoder, N=max_batch,
                        kernel_size=kernel_size)
            engine = Engine(dims, self.assembler, device)
            # models_shapes' decoder has no validity automaton: every token is valid at every step
            V = num_vocab_nmn
            engine.set_validity_tables(np.zeros((V, 3), np.int32), np.zeros((3, V, 4), np.int32),
                                       np.zeros((V, 4), np.int32))
        elif not getattr(engine, 'all_tokens_valid', False):
            # (a caller's engine keeps the tables it was given: installing the all-valid tables behind its back
            # would change what its other users decode)
            raise ValueError('models_shapes decodes without a validity automaton: give it an engine whose '
                             'set_validity_tables() installed all-zero tables, or let it build its own')
        self.engine = engine
        self.EOS_idx = EOS_idx
        self.T_decoder = T_decoder
        self.beam_size = int(beam_size)      # layouts by beam search of this width (the <eos> latch then runs per beam on the device)
        self.hidden_dim = hidden_dim
        self.image_batch = image_batch
        self.phase1_inputs = Phase1Inputs(text_seq_batch, seq_length_batch, use_gt_layout, gt_layout_batch)
        self._cnn = None
        for name in ('predicted_tokens', 'word_vecs', 'atts'):
            setattr(self, name, Fetch(self, name, 1))
        self.image_feat_grid = Fetch(self, 'image_feat_grid', 1)
        self.compiler = Compiler(self.assembler)
        self.scores = Fetch(self, 'scores', 2)
        register_model(self)

    # -- variables -------------------------------------------------------------------------------------
    def load_weights(self, weights):
        """reference-named variables of the models_shapes graph (oracle/n2nmn_oracle_shapes.variable_shapes
        lists them): the convnet's stay with the face, the seq2seq's go to the engine under their own names,
        the modules' under the engine's (<X>Module/<X>Module/... of the ScopedLayer naming ->
        module_variables/<X>Module/...; AnswerModule -> ExistModule); CLEVR variables models_shapes does not
        have are zero."""
        w = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in weights.items()}
        self._cnn = {k: np.ascontiguousarray(w[_CNN + k], np.float32)
                     for k in ('conv_1/weights', 'conv_1/biases', 'conv_2/weights', 'conv_2/biases')}
        out = {k: np.zeros(shp, np.float32) for k, shp in variable_shapes(self.engine.dims).items()}
        for k, v in w.items():
            if k.startswith(_MOD):
                name = k[len(_MOD):].split('/', 1)[1].replace('AnswerModule/', 'ExistModule/')
                k2 = _MOD + 'module_variables/' + name
            elif k.startswith(_CNN):
                continue
            else:
                k2 = k
            if k2 in out:
                if tuple(out[k2].shape) != tuple(v.shape):
                    raise ValueError('shape mismatch for %s: %s vs %s' % (k, v.shape, out[k2].shape))
                out[k2] = np.ascontiguousarray(v, np.float32)
        self.engine.load_weights(out)

    # -- eager execution -------------------------------------------------------------------------------
    def convnet(self, images):
        """shapes_convnet: [N, H_im, W_im, 3] (mean-subtracted) -> device tensor [N, H, W, feat_dim]"""
        torch = _torch()
        if self._cnn is None:
            raise RuntimeError('NMN3ModelAtt: weights not loaded')
        e, s = self.engine, self.stride
        x = e._dev(images, torch.float32)
        n, H, W = x.shape[0], self.H_im // s, self.W_im // s
        rows = x.reshape(n, H, s, W, s, self.C_im).permute(0, 1, 3, 2, 4, 5).reshape(n * H * W, s * s * self.C_im)
        k1 = self._cnn['conv_1/weights'].reshape(s * s * self.C_im, -1)
        c1 = e.fc(rows.contiguous(), k1, self._cnn['conv_1/biases'], relu=True)
        k2 = self._cnn['conv_2/weights']
        c2 = e.fc(c1, k2.reshape(k2.shape[2], k2.shape[3]), self._cnn['conv_2/biases'], relu=True)
        return c2.reshape(n, H, W, -1)

    def run_phase1(self, feeds=None):
        feeds = feeds or {}
        seq, lens, use_gt, gt = self.phase1_inputs.resolve(feeds)
        out = dict(self.engine.seq2seq(seq, lens, self.T_decoder, use_gt, gt, beam_size=self.beam_size))
        # the <eos> latch of models_shapes/nmn3_netgen_att.py:215-222: behind the first <eos> every token is <eos>
        tok = to_numpy(out['predicted_tokens']).copy()
        seen = np.cumsum(tok == self.EOS_idx, axis=0) > 0
        behind = np.vstack([np.zeros((1, tok.shape[1]), bool), seen[:-1]])
        tok[behind] = self.EOS_idx
        out['predicted_tokens'] = tok
        out['image_feat_grid'] = self.convnet(resolve(self.image_batch, feeds))
        return out

    def run_phase2(self, packed, feat, word_vecs):
        return self.engine.execute(packed, feat, word_vecs)

    def _fetch(self, f, handle):
        if handle.phase1 is None:
            handle.phase1 = self.run_phase1(handle.feeds)
        if f.phase == 1:
            return to_numpy(handle.phase1[f.name])
        if 'scores' not in handle.results:
            packed = resolve(self.compiler.loom_input_tensor, handle.feeds)
            handle.results['scores'] = self.run_phase2(packed, handle.phase1['image_feat_grid'],
                                                       handle.phase1['word_vecs'])
        return to_numpy(handle.results['scores'])


# ---------------------------------------------------------------------------------------------------------
# training: the N2NMN_VARIANT_SHAPES engine
VARIANT_SHAPES = 2                                       # include/n2nmn.h N2NMN_VARIANT_SHAPES
_ENGINE_MOD = _MOD + 'module_variables/'
# engine module scope -> the reference's (nmn3_model.py:60-80: td.ScopedLayer opens <X>Module twice)
_MODULE_SCOPES = {'FindModule': 'FindModule', 'TransformModule': 'TransformModule', 'ExistModule': 'AnswerModule'}


def reference_name(engine_name: str) -> str:
    """engine variable name -> models_shapes variable name (module_variables/<X>Module/... ->
    layout_execution/<Y>/<Y>/..., ExistModule -> AnswerModule); other names are shared"""
    if not engine_name.startswith(_ENGINE_MOD):
        return engine_name
    scope, rest = engine_name[len(_ENGINE_MOD):].split('/', 1)
    ref = _MODULE_SCOPES[scope]
    return _MOD + ref + '/' + ref + '/' + rest


def shapes_dims(num_vocab_txt: int, N: int = 256, T_encoder: int = 15, T_decoder: int = 11, lstm_dim: int = 256,
                embed_dim: int = 300, map_dim: int = 500, feat_dim: int = 64, num_choices: int = 2,
                H_im: int = 30, W_im: int = 30) -> Dims:
    """dimensions of the models_shapes training engine (defaults: exp_shapes/train_shapes_gt_layout.py:23-37)"""
    if H_im % 10 or W_im % 10:
        raise ValueError('image size must be a multiple of the 10x10 stride-10 kernel')
    return Dims(H=H_im // 10, W=W_im // 10, D=feat_dim, map_dim=map_dim, embed_dim_txt=embed_dim,
                embed_dim_nmn=embed_dim, lstm_dim=lstm_dim, num_layers=2, num_vocab_txt=num_vocab_txt,
                num_vocab_nmn=len(SHAPES_MODULE_NAMES), num_choices=num_choices, T_encoder=T_encoder,
                T_decoder=T_decoder, N=N, kernel_size=3, variant=VARIANT_SHAPES)


def shapes_engine_variable_shapes(d: Dims) -> dict:
    """engine name -> shape of the N2NMN_VARIANT_SHAPES variable table, in its order (host-side statement of
    csrc/capi.cpp build_vars for this variant: the seq2seq, the three modules models_shapes has, the convnet)"""
    full = variable_shapes(d)
    keep = ('FindModule/', 'TransformModule/', 'ExistModule/')
    out = {k: v for k, v in full.items()
           if not k.startswith(_ENGINE_MOD) or k[len(_ENGINE_MOD):].startswith(keep)}
    out[_CNN + 'conv_1/weights'] = (10, 10, 3, 64)
    out[_CNN + 'conv_1/biases'] = (64,)
    out[_CNN + 'conv_2/weights'] = (1, 1, 64, d.D)
    out[_CNN + 'conv_2/biases'] = (d.D,)
    return out


def l2_variables(names) -> set:
    """models_shapes/nmn3_model.py:104-108: the trainable variables under neural_module_network whose name ends
    in 'weights' (the set weight_decay * l2_reg covers; the engine applies the same rule to its own names)"""
    return {k for k in names if 'neural_module_network' in k and k.endswith('weights')}


def shapes_engine(num_vocab_txt: int, device: int = 0, **kw) -> Engine:
    """an Engine of the SHAPES variant, decoding without a validity automaton (all-valid tables)"""
    d = shapes_dims(num_vocab_txt, **kw)
    asm = _Assembler(list(SHAPES_MODULE_NAMES), op_code=SHAPES_OP_CODE, input_num=SHAPES_INPUT_NUM,
                     output_type=SHAPES_OUTPUT_TYPE)
    e = Engine(d, asm, device)
    V = d.num_vocab_nmn
    e.set_validity_tables(np.zeros((V, 3), np.int32), np.zeros((3, V, 4), np.int32), np.zeros((V, 4), np.int32))
    return e


class ShapesTrainer(Trainer):
    """One iteration of exp_shapes/train_shapes_gt_layout.py:143-163 on the GPU: shapes_convnet + the layout
    generator (teacher-forced, <eos> latch, encoder / decoder dropout on LSTM layer 0, keep_prob 0.5) + the
    modules; total = mean(CE) + mean(-log_seq_prob) + weight_decay * l2_reg; per-tensor clip_by_norm(10);
    Adam.  Every gradient, the convnet's included, is computed on the GPU.

    step(batch, gt_layout, dropout=None): batch holds image_batch [N, H_im, W_im, 3] (mean-subtracted),
    input_seq_batch [T, N], seq_length_batch [N], answer_label_batch [N].  dropout: None = multipliers drawn
    from the trainer's dropout_stream (seed) for the switched-on sites; False = no dropout for this step; or a
    dict {'enc0': [T, N, lstm_dim], 'dec0': [T_dec, N, lstm_dim]} of {0, 1} keep masks.  gradients() /
    get_weights() / load_weights() use the reference's models_shapes names.

    step_rl(batch, sample_uniforms, ...): one iteration of exp_shapes/train_shapes_scratch.py (policy gradient on
    sampled layouts; self.rl holds the driver's invalid_expr_loss 3, lambda_entropy 0.5, baseline_decay 0.99, and
    the baseline starts at 3)."""

    def __init__(self, engine: Engine, weight_decay: float = 5e-4, lr: float = 1e-3,
                 max_grad_l2_norm: float = 10.0, encoder_dropout: bool = True, decoder_dropout: bool = True,
                 keep_prob: float = 0.5, seed: int = 0, dist=None, rccl=None):
        if engine.dims.variant != VARIANT_SHAPES:
            raise ValueError('ShapesTrainer needs an engine of the SHAPES variant (shapes_engine())')
        super().__init__(engine, weight_decay=weight_decay, lr=lr, max_grad_l2_norm=max_grad_l2_norm,
                         dist=dist, rccl=rccl)
        self.dropout = dict(enc0=bool(encoder_dropout), dec0=bool(decoder_dropout))
        self.dropout_stream.keep_prob = float(keep_prob)
        self.dropout_stream.seed = int(seed)
        self.ref_layout = {reference_name(k): v for k, v in self.layout.items()}
        # exp_shapes/train_shapes_scratch.py:39-43,144: the baseline starts at invalid_expr_loss
        self.rl = dict(invalid_expr_loss=3.0, lambda_entropy=0.5, baseline_decay=0.99)
        self.set_baseline(self.rl['invalid_expr_loss'])
        self._tokens = None              # [T_dec, N] tokens of the last sampling pass (device)

    def _io(self, batch, *args):
        return super()._io(dict(batch, image_feat_batch=batch['image_batch']), *args)

    def step_rl(self, batch, sample_uniforms, lr=None, update: bool = True, dropout=None):
        """One iteration of exp_shapes/train_shapes_scratch.py:204-232.  n2nmn_train_sample runs shapes_convnet,
        the encoder and the decoder once, sampling a layout per question (sample_uniforms [T_dec, N] in [0, 1)
        replace tf.multinomial's generator) under this step's dropout multipliers and the <eos> latch, with the
        activations kept; the tokens are fetched and assembled on the host (the reference's partial_run does the
        same); the module network, the policy-gradient loss, both backward phases and Adam follow.  lr=None: the
        trainer's own rate (the driver has no fine-tuning rate); update=False: losses and gradients only.
        Returns (losses, tokens, expr_validity)."""
        torch = _torch()
        e = self.engine
        seq = e._dev(batch['input_seq_batch'], torch.int32)
        lens = e._dev(batch['seq_length_batch'], torch.int32)
        img = e._dev(batch['image_batch'], torch.float32)
        T, N = seq.shape
        Td = self.ref_dims.T_decoder
        uni = e._dev(sample_uniforms, torch.float32)
        if tuple(uni.shape) != (Td, N):
            raise ValueError('sample_uniforms: shape %s, expected %s' % (tuple(uni.shape), (Td, N)))
        mult = self.multipliers(T, N, Td, dropout)
        if self._tokens is None or tuple(self._tokens.shape) != (Td, N):
            self._tokens = torch.empty((Td, N), dtype=torch.int32, device=e.device)
        io = _lib.TrainIO()
        io.input_seq = seq.data_ptr(); io.seq_length = lens.data_ptr(); io.image_feat = img.data_ptr()
        io.T_enc = T; io.N = N; io.T_dec = Td
        for key, m in mult.items():
            setattr(io, DROPOUT_FIELDS[key], m.data_ptr())
        _lib.check(self._lib.n2nmn_train_sample(self._ctx, C.byref(io), uni.data_ptr(), self._tokens.data_ptr(),
                                                e.stream()))
        tokens = self._tokens.cpu().numpy()
        batch = dict(batch, input_seq_batch=seq, seq_length_batch=lens, image_batch=img)
        scale = self._forward_backward(batch, tokens, True, 2, mult=mult, gt_dev=self._tokens)
        if update:
            saved = self.hyper['lr']
            self.hyper['lr'] = saved if lr is None else float(lr)
            self.apply(scale)
            self.hyper['lr'] = saved
        return self.losses, tokens, self.last_validity.copy()

    # -- reference names ---------------------------------------------------------------------------------
    def gradients(self):
        return {reference_name(k): v for k, v in super().gradients().items()}

    def get_weights(self):
        return {reference_name(k): v for k, v in super().get_weights().items()}

    def load_weights(self, weights):
        """models_shapes-named variables (oracle/n2nmn_oracle_shapes.variable_shapes lists them)"""
        inv = {reference_name(k): k for k in self.layout}
        missing = sorted(set(inv) - set(weights))
        extra = sorted(set(weights) - set(inv))
        if missing or extra:
            raise KeyError('models_shapes variables: missing %s, unknown %s' % (missing[:4], extra[:4]))
        self.engine.load_weights({inv[k]: v for k, v in weights.items()})

    def _state_variables(self):
        """optimizer_state() / load_optimizer_state() use the models_shapes names too"""
        return {k: (reference_name(k), tuple(shape)) for k, (_, _, shape) in self.layout.items()}


__all__ = ['Assembler', 'NMN3ModelAtt', 'SHAPES_MODULE_NAMES', 'ShapesTrainer', 'shapes_engine', 'shapes_dims',
           'reference_name', 'shapes_engine_variable_shapes', 'l2_variables']
