"""Host side of the training step (BASELINE.json configs[3]): the loop body of
exp_clevr/train_clevr_gt_layout.py:150-200 -- forward of the behavioural-cloning objective with
ground-truth layouts, backward, per-tensor clip-by-norm, Adam -- on top of the C-ABI
(include/n2nmn.h section 6), plus the data-parallel gradient exchange the reference does not have
(SURVEY.md 8e): one flat fp32 gradient buffer, all-reduced in two buckets so that the decoder +
module bucket travels over RCCL while the encoder's backward pass is still running.

PyTorch is plumbing only (device buffers, streams, torch.distributed); all arithmetic is in
libn2nmn_hip.so and there is no fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import _lib
from .engine import Engine


def _torch():
    import torch
    return torch


BWD_DEFER_JOIN = 0x10          # include/n2nmn.h
# dropout site -> its field of n2nmn_train_io, in the order the multipliers are drawn
DROPOUT_FIELDS = dict(enc0='drop_enc0', dec0='drop_dec0', qpn_h='drop_qpn_h', qpn_fc1='drop_qpn_fc1')


# ---- optimiser state: the names a TensorFlow 1.0.0 Saver gives Adam's variables (restated from
# tensorflow/python/training/adam.py and slot_creator.py: slots `<variable>/Adam` = m and `<variable>/Adam_1` = v,
# non-slot `beta1_power` / `beta2_power` that START at beta and are multiplied by beta after every step), plus
# two entries of this package's own for what TensorFlow keeps nowhere a Saver reaches
ADAM_STEP_KEY = 'n2nmn_amd/adam_step'
DROPOUT_OFFSET_KEY = 'n2nmn_amd/dropout_offset'
_SCALAR_KEYS = ('beta1_power', 'beta2_power', ADAM_STEP_KEY, DROPOUT_OFFSET_KEY)


def slot_names(variable: str):
    """(first moment, second moment) entries of one variable"""
    return variable + '/Adam', variable + '/Adam_1'


def optimizer_state_keys(variables) -> list:
    """every key of Trainer.optimizer_state() for reference-named `variables`, in its order"""
    return [s for v in variables for s in slot_names(v)] + list(_SCALAR_KEYS)


def is_optimizer_state_key(key: str, variables) -> bool:
    """`key` is an optimiser entry of a model whose variables are `variables` (a set)"""
    if key in _SCALAR_KEYS:
        return True
    for suffix in ('/Adam', '/Adam_1'):
        if key.endswith(suffix) and key[:-len(suffix)] in variables:
            return True
    return False


def beta_powers(iteration: int, beta1: float, beta2: float):
    """(beta1_power, beta2_power) after `iteration` steps, float32: beta ** (iteration + 1) of the float32 beta
    the update itself uses (TensorFlow holds both as float32 variables)."""
    t = int(iteration) + 1
    return tuple(np.float32(float(np.float32(b)) ** t) for b in (beta1, beta2))


def step_drift_bound(iteration: int, beta2: float) -> int:
    """How many steps iteration_from_state() may be off for a `beta2_power` that TensorFlow accumulated as a
    float32 product (derivation there): ceil(iteration * 2^-24 / |ln beta2|) once that exceeds 1/2, else 0."""
    d = int(iteration) * 2.0 ** -24 / abs(np.log(float(np.float32(beta2))))
    return 0 if d < 0.5 else int(np.ceil(d))


def iteration_from_state(state, beta2: float) -> int:
    """The number of steps taken, from an optimiser state: its ADAM_STEP_KEY entry when it has one (files this
    package wrote), else round(log(beta2_power) / log(beta2)) - 1 (files TensorFlow wrote).  beta1_power is
    never used: at 0.9 it leaves float32's range after roughly 900 steps.

    The second form is exact for short runs and APPROXIMATE for long ones.  TensorFlow's beta2_power is
    fl(beta2) times itself t more times in float32, every product rounded with relative error <= u = 2^-24,
    so it equals beta2^(t+1) * prod(1 + e_i) with |e_i| <= u and the recovered exponent is off by at most
    t * u / |ln beta2| steps.  At beta2 = 0.999 that is t * 5.96e-5: below 1/2, i.e. rounded away, for every
    t < 8393, and at most 5 steps at t = 80000 (step_drift_bound).  It is harmless there because the step count
    enters the update only through lr_t / lr = sqrt(1 - beta2^t) / (1 - beta1^t): a drift of d steps changes
    beta2^t by the factor beta2^d, so the square root moves by about beta2^t * d * |ln beta2| / 2
    <= beta2^t * t * u / 2.  With t * beta2^t <= 1 / (e * |ln beta2|) = 368 that is never more than 1.1e-5
    relative (reached near t = 1000, where d rounds to zero anyway).  Where d can be nonzero (t >= 8393) the
    bound beta2^t * t * u / 2 is 5.7e-8 already, under float32's resolution u, and falls off as e^(-t/1000):
    at t = 80000 beta2^t = 1.7e-35 and the factor differs from 1 by about 4e-38 whatever d is; beta1^t
    underflowed long before.  A beta2_power that has underflowed to zero (t beyond ~103 000) gives the first
    step count at which float32 does so; the same argument covers it."""
    if ADAM_STEP_KEY in state:
        return int(np.asarray(state[ADAM_STEP_KEY]).reshape(-1)[0])
    if 'beta2_power' not in state:
        raise KeyError('optimizer state: neither %s nor beta2_power' % ADAM_STEP_KEY)
    b2p = float(np.asarray(state['beta2_power'], np.float64).reshape(-1)[0])
    lb = np.log(float(np.float32(beta2)))
    if not (b2p < 1.0) or lb >= 0.0:
        raise ValueError('optimizer state: beta2_power %r is not a power of beta2 = %r' % (b2p, beta2))
    if b2p <= 0.0:
        return int(np.ceil(np.log(2.0 ** -150) / lb))
    return max(int(round(np.log(b2p) / lb)) - 1, 0)


class DropoutStream:
    """Dropout multipliers (0 or 1 / keep_prob per element) of one model: from {0, 1} keep masks, or drawn
    on the device from the library's counter-based stream at (seed, offset), each draw taking a fresh
    stretch of it."""

    def __init__(self, engine: Engine, keep_prob: float = 0.5, seed: int = 0):
        self.engine = engine
        self.keep_prob = float(keep_prob)
        self.seed = int(seed)
        self.offset = 0

    def multipliers(self, shapes, masks=None):
        """shapes: ordered {site: shape} of the switched-on sites.  masks None: draw each site in order;
        False: no dropout ({}); a dict of keep masks: keep / keep_prob for each site it holds (a missing or
        None site gets no multiplier, a site not in `shapes` is ignored).  Returns float32 device tensors."""
        torch = _torch()
        e = self.engine
        out = {}
        if masks is False:
            return out
        for key, shape in shapes.items():
            if masks is None:
                m = torch.empty(shape, dtype=torch.float32, device=e.device)
                _lib.check(e._lib.n2nmn_dropout_multipliers(m.data_ptr(), m.numel(), self.keep_prob, self.seed,
                                                            self.offset, e.stream()))
                self.offset += m.numel()
            elif masks.get(key) is not None:
                keep = torch.as_tensor(np.asarray(masks[key], np.float32), device=e.device)
                if tuple(keep.shape) != tuple(shape):
                    raise ValueError('dropout mask %s: shape %s, expected %s' % (key, tuple(keep.shape), tuple(shape)))
                m = (keep / self.keep_prob).contiguous()
            else:
                continue
            out[key] = m
        return out


class GradBuckets:
    """Two-bucket all-reduce of a flat gradient vector (sum over ranks; the optimiser applies the
    1/world scale).  `late` = [split, numel) is ready first (decoder + modules), `early` =
    [0, split) (encoder) last.  Works on any torch.distributed backend (RCCL on GPUs, gloo in
    the CPU tests); without a process group it is a no-op."""

    def __init__(self, flat, split: int, dist=None):
        self.flat = flat
        self.split = int(split)
        self.dist = dist
        self._pending = []

    @property
    def world(self) -> int:
        return self.dist.get_world_size() if self.dist is not None else 1

    def reduce_late(self):
        if self.dist is not None:          # (a 1-rank group still goes through the collective)
            self._pending.append(self.dist.all_reduce(self.flat[self.split:], async_op=True))

    def reduce_early(self):
        if self.dist is not None:
            self._pending.append(self.dist.all_reduce(self.flat[:self.split], async_op=True))

    def wait(self) -> float:
        """Blocks the current stream on both collectives; returns the scale that turns the sum into
        the mean over ranks."""
        for w in self._pending:
            w.wait()
        self._pending = []
        return 1.0 / self.world


class RcclBuckets:
    """The same two buckets through the C-ABI's own RCCL communicator (n2nmn_comm_create /
    n2nmn_allreduce_grads / n2nmn_allreduce_wait, include/n2nmn.h section 6b): the collectives run
    on a library-owned side stream forked from and joined to the caller's stream with events.
    torch.distributed is used for ONE thing only: handing rank 0's 128-byte ncclUniqueId to the other
    ranks.  dist=None: a 1-rank communicator (the code path of the 8-GPU run on one GPU)."""

    def __init__(self, engine: Engine, flat, dist=None):
        torch = _torch()
        self.engine, self.flat, self.dist = engine, flat, dist
        self._lib = engine._lib
        self.rank = dist.get_rank() if dist is not None else 0
        self._world = dist.get_world_size() if dist is not None else 1
        uid = (C.c_char * 128)()
        if self.rank == 0:
            _lib.check(self._lib.n2nmn_comm_unique_id(uid))
        if dist is not None and self._world > 1:
            box = [bytes(uid.raw) if self.rank == 0 else None]
            dist.broadcast_object_list(box, src=0, device=engine.device)
            C.memmove(uid, box[0], 128)
        self._comm = C.c_void_p()
        _lib.check(self._lib.n2nmn_comm_create(uid, self.rank, self._world, engine.device.index,
                                               C.byref(self._comm)))
        torch.cuda.synchronize(engine.device)
        self.verified_world = self._self_test()

    def _self_test(self) -> int:
        """One all-reduce of both buckets over a buffer of ones, through the very calls a step uses:
        every element must come back as the number of ranks.  Proves at construction that the
        communicator spans `world` ranks (the figure bench.py prints as `rccl_ranks`) instead of
        assuming it from WORLD_SIZE; leaves the gradient buffer zeroed."""
        torch = _torch()
        self.flat.fill_(1.0)
        self.reduce_late()
        self.reduce_early()
        self.wait()
        torch.cuda.synchronize(self.engine.device)
        lo, hi = float(self.flat.min().item()), float(self.flat.max().item())
        self.flat.zero_()
        if lo != hi or int(lo) != self.comm_world():
            raise RuntimeError('RCCL self-test: all-reduce of ones over %d ranks returned [%g, %g]' %
                               (self._world, lo, hi))
        return int(lo)

    def comm_world(self) -> int:
        """ranks of the C-ABI communicator as the library reports them (n2nmn_comm_world)"""
        return int(_lib.check(self._lib.n2nmn_comm_world(self._comm)))

    @property
    def world(self) -> int:
        return self._world

    def reduce_late(self):
        _lib.check(self._lib.n2nmn_allreduce_grads(self.engine._ctx, self._comm, 0,
                                                   self.flat.data_ptr(), self.engine.stream()))

    def reduce_early(self):
        _lib.check(self._lib.n2nmn_allreduce_grads(self.engine._ctx, self._comm, 1,
                                                   self.flat.data_ptr(), self.engine.stream()))

    def wait(self) -> float:
        _lib.check(self._lib.n2nmn_allreduce_wait(self._comm, self.engine.stream()))
        return 1.0 / self._world

    def close(self):
        comm, self._comm = self._comm, None
        if comm:
            self._lib.n2nmn_comm_destroy(comm)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_rccl(dist) -> bool:
    """Which all-reduce a Trainer uses when the caller does not say: the C-ABI communicator
    (side-stream all-reduce under the encoder's backward pass) on every nccl (= RCCL) group, one
    rank or many -- tests/test_gpu_rccl_multi.py checks gradient equality across ranks on it wherever
    a node has >= 2 devices, and its constructor proves the rank count with an all-reduce of ones.
    N2NMN_RCCL_BUCKETS=0 selects torch.distributed's all_reduce instead; gloo groups always use it."""
    import os
    return dist is not None and dist.get_backend() == 'nccl' and \
        os.environ.get('N2NMN_RCCL_BUCKETS', '1') != '0'


class Trainer:
    """One model replica on one GPU.  `step(batch, gt_layout)` = one iteration of
    train_clevr_gt_layout.py: returns the losses of that iteration (device tensor of 4 floats:
    avg_sample_loss, seq_likelihood_loss, l2_reg, total_loss)."""

    def __init__(self, engine: Engine, weight_decay: float = 5e-6, lr: float = 1e-3,
                 beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 max_grad_l2_norm: float = 10.0, dist=None, rccl: Optional[bool] = None):
        """dist: an initialised torch.distributed module (or None).  rccl: all-reduce through the
        C-ABI's own RCCL communicator (n2nmn_comm_* / n2nmn_allreduce_grads); False / gloo:
        torch.distributed collectives.  Default: the C-ABI communicator on every nccl group
        (N2NMN_RCCL_BUCKETS=0 opts out); `bucket_impl` / `rccl_ranks` say what a trainer runs on."""
        torch = _torch()
        if engine._parent is not None:
            raise ValueError('train on the root engine, not on a fork')
        self.engine = engine
        self._lib = engine._lib
        self._ctx = engine._ctx
        _lib.check(self._lib.n2nmn_train_enable(self._ctx))
        self.numel = int(self._lib.n2nmn_grad_numel(self._ctx))
        self.split = int(self._lib.n2nmn_grad_split(self._ctx))
        self.weight_decay = float(weight_decay)
        self.hyper = dict(lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps),
                          max_grad_l2_norm=float(max_grad_l2_norm))
        self.grads = torch.zeros(self.numel, dtype=torch.float32, device=engine.device)
        # avg_sample_loss, seq_likelihood | policy_gradient loss, l2_reg, total_loss, entropy_reg, -
        self.losses = torch.zeros(8, dtype=torch.float32, device=engine.device)
        # policy gradient (train_clevr_rl_gt_layout.py:38-42,120): baseline starts at
        # invalid_expr_loss and is an EMA of avg_sample_loss, kept on the device
        self.rl = dict(invalid_expr_loss=0.5, lambda_entropy=0.005, baseline_decay=0.99)
        self.baseline = torch.full((1,), self.rl['invalid_expr_loss'], dtype=torch.float32,
                                   device=engine.device)
        self.scores = None
        self.last_validity = None
        if rccl is None:
            rccl = default_rccl(dist)
        self.buckets = RcclBuckets(engine, self.grads, dist) if rccl else \
            GradBuckets(self.grads, self.split, dist)
        self.bucket_impl = 'n2nmn_comm (C-ABI RCCL communicator, library side stream)' if rccl else \
            ('torch.distributed.all_reduce (%s)' % dist.get_backend() if dist is not None else 'none (one process)')
        self.rccl_ranks = self.buckets.verified_world if rccl else None
        self.iteration = 0
        _lib.check(self._lib.n2nmn_train_reset_optimizer(self._ctx, engine.stream()))
        self.layout: Dict[str, tuple] = {}
        names = list(engine.variable_names().items())
        for i, (name, shape) in enumerate(names):
            off, n = C.c_int64(), C.c_int64()
            _lib.check(self._lib.n2nmn_grad_layout(self._ctx, i, C.byref(off), C.byref(n)))
            self.layout[name] = (int(off.value), int(n.value), shape)
        self._keep = None
        # dropout: site -> switched on (CLEVR: no site); the shapes of the masks follow the reference's dims
        self.dropout: Dict[str, bool] = {}
        self.ref_dims = engine.dims
        self.dropout_stream = DropoutStream(engine)
        self._mult = None                # the last step's multipliers

    # ------------------------------------------------------------------------------------
    def dropout_shapes(self, T: int, N: int, Td: int) -> Dict[str, tuple]:
        """reference shape of every switched-on dropout site, in the order the multipliers are drawn"""
        d = self.ref_dims
        L = d.lstm_dim
        shapes = dict(enc0=(T, N, L), dec0=(Td, N, L), qpn_h=(N, d.num_layers * L), qpn_fc1=(N, d.qpn_hidden))
        return {k: shapes[k] for k in DROPOUT_FIELDS if self.dropout.get(k)}

    def _pad_multiplier(self, key: str, m):
        """reference-shaped multiplier -> the context's layout (identity unless the context pads)"""
        return m

    def multipliers(self, T: int, N: int, Td: int, dropout=None) -> Dict[str, object]:
        """this step's dropout multipliers in the context's layout.  dropout: None = drawn from
        self.dropout_stream; False = none; or a dict of reference-shaped {0, 1} keep masks."""
        mult = self.dropout_stream.multipliers(self.dropout_shapes(T, N, Td), dropout)
        return {k: self._pad_multiplier(k, m) for k, m in mult.items()}

    def _io(self, batch, gt_layout, objective: int = 0, dropout=None, mult=None, gt_dev=None):
        """gt_dev: the device copy of gt_layout where one exists already (tokens sampled on the device)"""
        torch = _torch()
        e = self.engine
        d = e.dims
        seq = e._dev(batch['input_seq_batch'], torch.int32)
        lens = e._dev(batch['seq_length_batch'], torch.int32)
        feat = e._dev(batch['image_feat_batch'], torch.float32)
        labels = e._dev(batch['answer_label_batch'], torch.int32)
        gt_host = np.ascontiguousarray(np.asarray(
            gt_layout.cpu().numpy() if hasattr(gt_layout, 'cpu') else gt_layout), np.int32)
        # pinned slot: no stream synchronisation per step
        gt = e.upload_i32(gt_host) if gt_dev is None else gt_dev
        T, N = seq.shape
        Td = gt.shape[0]
        # teacher forcing: the layout is known before the forward, so the program is assembled
        # up front and there is no host sync inside the step
        packed, validity = e.assembler.assemble_packed(gt_host)
        if self.scores is None or tuple(self.scores.shape) != (N, d.num_choices):
            self.scores = torch.empty((N, d.num_choices), dtype=torch.float32, device=e.device)
        io = _lib.TrainIO()
        io.input_seq = seq.data_ptr(); io.seq_length = lens.data_ptr()
        io.T_enc = T; io.N = N; io.T_dec = Td
        io.gt_layout = gt.data_ptr(); io.image_feat = feat.data_ptr()
        io.answer_labels = labels.data_ptr(); io.weight_decay = self.weight_decay
        io.scores = self.scores.data_ptr(); io.losses = self.losses.data_ptr()
        io.grads = self.grads.data_ptr()
        val = None
        if objective != 0:               # policy gradient (1; 2: on layouts sampled inside this step)
            val = e.upload_i32(np.asarray(validity, np.int32))
            io.objective = objective
            io.expr_validity = val.data_ptr()
            io.invalid_expr_loss = self.rl['invalid_expr_loss']
            io.lambda_entropy = self.rl['lambda_entropy']
            io.baseline_decay = self.rl['baseline_decay']
            io.baseline = self.baseline.data_ptr()
        self._mult = self.multipliers(T, N, Td, dropout) if mult is None else mult
        for key, m in self._mult.items():
            setattr(io, DROPOUT_FIELDS[key], m.data_ptr())
        self._keep = (seq, lens, feat, labels, gt, packed, val)
        self.last_validity = np.asarray(validity, bool)
        return io, packed, validity

    def forward_backward(self, batch, gt_layout, reduce: bool = True, objective: int = 0, dropout=None) -> float:
        """Forward + both backward phases (+ the bucketed all-reduce).  Afterwards self.grads is
        d total_loss / d variables summed over ranks; returns the 1/world scale.
        objective 0: behavioural cloning on ground-truth layouts; 1: policy gradient, gt_layout
        then being the layout the decoder sampled for this batch (see step_rl).
        dropout: as for multipliers() (None: drawn, if the trainer has dropout sites)."""
        return self._forward_backward(batch, gt_layout, reduce, objective, dropout)

    def _forward_backward(self, batch, gt_layout, reduce, objective, dropout=None, mult=None, gt_dev=None) -> float:
        """mult: ready multipliers (step_rl: the ones the layout was sampled under) instead of `dropout`"""
        io, packed, _ = self._io(batch, gt_layout, objective, dropout, mult, gt_dev)
        s = self.engine.stream()
        _lib.check(self._lib.n2nmn_train_forward(self._ctx, C.byref(io), packed.handle, s))
        # the decoder's weight gradients and the finish of the late bucket stay on the library's side
        # stream under the encoder's backward pass (N2NMN_BWD_DEFER_JOIN, include/n2nmn.h).  A
        # torch.distributed all-reduce knows nothing of that stream: the caller's stream joins it first.
        torch_reduce = reduce and isinstance(self.buckets, GradBuckets) and self.buckets.dist is not None
        _lib.check(self._lib.n2nmn_train_backward(self._ctx, C.byref(io), packed.handle,
                                                  0 | BWD_DEFER_JOIN, s))
        if torch_reduce:
            _lib.check(self._lib.n2nmn_train_join(self._ctx, s))
        if reduce:
            self.buckets.reduce_late()       # overlaps the encoder's backward pass
        _lib.check(self._lib.n2nmn_train_backward(self._ctx, C.byref(io), packed.handle, 1, s))
        if reduce:
            self.buckets.reduce_early()
            return self.buckets.wait()
        return 1.0

    def set_baseline(self, value: float):
        """the REINFORCE baseline (train_clevr_rl_gt_layout.py:120: tf.Variable(invalid_expr_loss))"""
        self.baseline.fill_(float(value))

    def get_baseline(self) -> float:
        return float(self.baseline.item())

    def apply(self, scale: float = 1.0):
        self.iteration += 1
        h = self.hyper
        _lib.check(self._lib.n2nmn_adam_step(self._ctx, self.grads.data_ptr(), scale, h['lr'],
                                             h['beta1'], h['beta2'], h['eps'],
                                             h['max_grad_l2_norm'], self.iteration,
                                             self.engine.stream()))

    def step(self, batch, gt_layout, dropout=None):
        scale = self.forward_backward(batch, gt_layout, dropout=dropout)
        self.apply(scale)
        return self.losses

    def step_rl(self, batch, sample_uniforms, lr: Optional[float] = 1e-4, update: bool = True, dropout=None):
        """One iteration of exp_clevr/train_clevr_rl_gt_layout.py:183-214 (exp_vqa/train_vqa_rl_gt_layout.py:
        150-196): the decoder samples a layout per question (sample_uniforms [T_dec, N] in [0,1) replace
        tf.multinomial's RNG) under this step's dropout multipliers (the reference samples inside the
        training graph), the tokens are fetched and assembled on the host (the reference's partial_run
        does the same), then forward + backward of the policy-gradient loss under the same multipliers
        and an Adam step with the fine-tuning learning rate (lr=None: the trainer's own).  update=False
        computes the losses and gradients only (no Adam step).  Returns (losses, tokens, expr_validity)."""
        torch = _torch()
        T, N = torch.as_tensor(batch['input_seq_batch']).shape
        Td = self.ref_dims.T_decoder
        mult = self.multipliers(T, N, Td, dropout)
        s2s = self.engine.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], Td,
                                  sample_uniforms=sample_uniforms, dropout=(mult.get('enc0'), mult.get('dec0')))
        tokens = s2s['predicted_tokens'].cpu().numpy()
        scale = self._forward_backward(batch, tokens, True, 1, mult=mult)
        if update:               # lr=None: the trainer's own learning rate
            saved = self.hyper['lr']
            self.hyper['lr'] = saved if lr is None else float(lr)
            self.apply(scale)
            self.hyper['lr'] = saved
        validity = self._keep[6].cpu().numpy().astype(bool) if self._keep[6] is not None else None
        return self.losses, tokens, validity

    # ------------------------------------------------------------------------------------
    def gradients(self) -> Dict[str, object]:
        """name -> view of the flat gradient buffer in the variable's reference shape."""
        return {name: self.grads[off:off + n].view(shape)
                for name, (off, n, shape) in self.layout.items()}

    def get_weights(self) -> Dict[str, object]:
        torch = _torch()
        out = {}
        for name, (off, n, shape) in self.layout.items():
            t = torch.empty(shape, dtype=torch.float32, device=self.engine.device)
            _lib.check(self._lib.n2nmn_get_weight(self._ctx, name.encode(), t.data_ptr(),
                                                  self.engine.stream()))
            out[name] = t
        return out

    # -- optimiser state ---------------------------------------------------------------------------
    def _state_variables(self) -> Dict[str, tuple]:
        """engine variable name -> (reference name, reference shape) of its optimiser entries"""
        return {name: (name, tuple(shape)) for name, (_, _, shape) in self.layout.items()}

    def _state_to_reference(self, name: str, a: np.ndarray) -> np.ndarray:
        """engine-shaped moment of engine variable `name` -> reference shape (identity unless the context pads)"""
        return a

    def _state_from_reference(self, name: str, a: np.ndarray) -> np.ndarray:
        return a

    def _read_moments(self):
        """(m, v): host copies of the flat moment vectors"""
        torch = _torch()
        e = self.engine
        m = torch.empty(self.numel, dtype=torch.float32, device=e.device)
        v = torch.empty(self.numel, dtype=torch.float32, device=e.device)
        _lib.check(self._lib.n2nmn_train_get_moments(self._ctx, m.data_ptr(), v.data_ptr(), e.stream()))
        torch.cuda.synchronize(e.device)
        return m.cpu().numpy(), v.cpu().numpy()

    def _write_moments(self, m: np.ndarray, v: np.ndarray):
        torch = _torch()
        e = self.engine
        md = torch.as_tensor(m).to(device=e.device, dtype=torch.float32).contiguous()
        vd = torch.as_tensor(v).to(device=e.device, dtype=torch.float32).contiguous()
        _lib.check(self._lib.n2nmn_train_set_moments(self._ctx, md.data_ptr(), vd.data_ptr(), e.stream()))
        torch.cuda.synchronize(e.device)     # (md / vd live until the copies are done)

    def optimizer_state(self) -> Dict[str, np.ndarray]:
        """What a TensorFlow 1.0.0 Saver stores for tf.train.AdamOptimizer besides the variables, as host arrays
        (the keys of optimizer_state_keys): `<name>/Adam` (m) and `<name>/Adam_1` (v) per variable, reference-named
        and reference-shaped float32; `beta1_power` / `beta2_power` = beta ** (iteration + 1), float32 scalars;
        and, int64 scalars of this package's own, the step count and the dropout stream's offset.  The REINFORCE
        `baseline` is not part of it (the reference's fine-tuning scripts leave it out of what they restore,
        train_clevr_rl_gt_layout.py:178-179): get_baseline / set_baseline."""
        m, v = self._read_moments()
        out: Dict[str, np.ndarray] = {}
        for name, (ref, _) in self._state_variables().items():
            off, n, shape = self.layout[name]
            km, kv = slot_names(ref)
            out[km] = np.ascontiguousarray(self._state_to_reference(name, m[off:off + n].reshape(shape)), np.float32)
            out[kv] = np.ascontiguousarray(self._state_to_reference(name, v[off:off + n].reshape(shape)), np.float32)
        out['beta1_power'], out['beta2_power'] = beta_powers(self.iteration, self.hyper['beta1'], self.hyper['beta2'])
        out[ADAM_STEP_KEY] = np.int64(self.iteration)
        out[DROPOUT_OFFSET_KEY] = np.int64(self.dropout_stream.offset)
        return out

    def load_optimizer_state(self, state, strict: bool = True):
        """Inverse of optimizer_state(): sets the moments, `iteration` (iteration_from_state: the stored step
        count, else recovered from beta2_power -- approximate for long runs, see there) and, where present, the
        dropout stream's offset.  strict=False leaves the moments of a variable at zero when BOTH its entries
        are absent and, without any step entry, the iteration as it is; entries of other names are ignored.
        A wrong-shaped entry raises ValueError naming the variable."""
        m = np.zeros(self.numel, np.float32)
        v = np.zeros(self.numel, np.float32)
        for name, (ref, ref_shape) in self._state_variables().items():
            off, n, shape = self.layout[name]
            keys = slot_names(ref)
            have = [k in state for k in keys]
            if not any(have) and not strict:
                continue
            if not all(have):
                raise KeyError('optimizer state: no entry %s' % keys[have.index(False)])
            for k, flat in zip(keys, (m, v)):
                a = np.asarray(state[k], np.float32)
                if tuple(a.shape) != ref_shape:
                    raise ValueError('optimizer state %s: shape %s, the variable %s is %s'
                                     % (k, tuple(a.shape), ref, ref_shape))
                flat[off:off + n] = np.asarray(self._state_from_reference(name, a), np.float32).reshape(-1)
        if strict or ADAM_STEP_KEY in state or 'beta2_power' in state:
            iteration = iteration_from_state(state, self.hyper['beta2'])
        else:
            iteration = self.iteration
        self._write_moments(m, v)
        self.iteration = iteration
        if DROPOUT_OFFSET_KEY in state:
            self.dropout_stream.offset = int(np.asarray(state[DROPOUT_OFFSET_KEY]).reshape(-1)[0])

    def debug_tensor(self, name: str, shape):
        torch = _torch()
        n = int(np.prod(shape))
        t = torch.empty(n, dtype=torch.float32, device=self.engine.device)
        got = self._lib.n2nmn_train_debug_tensor(self._ctx, name.encode(), t.data_ptr(), n,
                                                 self.engine.stream())
        _lib.check(int(got))
        return t[:int(got)].view(shape) if int(got) == n else t[:int(got)]
