"""Optimiser state (Trainer.optimizer_state / load_optimizer_state, the Saver's handling of Adam's slots), host
side: names, the step count recovered from the beta powers, the checkpoint round trip and the restore that waits
for its trainer.  The trainers here are the real classes with the two methods that touch the device
(_read_moments / _write_moments) answered from numpy arrays; tests/test_gpu_optimizer_state.py runs them on the GPU.
"""
import re
import types

import numpy as np
import pytest

from n2nmn_amd import runtime, runtime_train, tf_checkpoint
from n2nmn_amd import train as T
from n2nmn_amd.models_shapes import reference_name, shapes_dims, shapes_engine_variable_shapes, ShapesTrainer
from n2nmn_amd.spec import Dims, variable_shapes
from n2nmn_amd.vqa import VQADims, VQATrainer, internal_dims, pad_variable, vqa_variable_shapes


class _Host:
    """a Trainer without a device: `shapes` is the engine's variable table (name -> shape)"""

    def __init__(self, shapes, beta1=0.9, beta2=0.999):
        self.layout, off = {}, 0
        for name, shape in shapes.items():
            n = int(np.prod(shape))
            self.layout[name] = (off, n, tuple(shape))
            off += n
        self.numel = off
        self.hyper = dict(lr=1e-3, beta1=beta1, beta2=beta2, eps=1e-8, max_grad_l2_norm=10.0)
        self.iteration = 0
        self.dropout_stream = types.SimpleNamespace(offset=0)
        self.m = np.zeros(off, np.float32)        # (a constructor resets the optimiser)
        self.v = np.zeros(off, np.float32)

    def _read_moments(self):
        return self.m.copy(), self.v.copy()

    def _write_moments(self, m, v):
        self.m, self.v = np.array(m, np.float32), np.array(v, np.float32)

    def fill(self, seed, iteration, offset=0):
        rng = np.random.default_rng(seed)
        self.m = rng.standard_normal(self.numel).astype(np.float32)
        self.v = rng.random(self.numel).astype(np.float32)
        self.iteration, self.dropout_stream.offset = iteration, offset


class HostTrainer(_Host, T.Trainer):
    pass


class HostShapesTrainer(_Host, ShapesTrainer):
    pass


class HostVQATrainer(_Host, VQATrainer):
    def __init__(self, d):
        self.vqa = types.SimpleNamespace(dims=d, idims=internal_dims(d))
        ref = vqa_variable_shapes(d)
        _Host.__init__(self, {k: pad_variable(k, np.zeros(s, np.float32), d, self.vqa.idims).shape
                              for k, s in ref.items()})

    def fill(self, seed, iteration, offset=0):
        # the moments of padding elements are zero on a device (zero gradient at every step)
        _Host.fill(self, seed, iteration, offset)
        for name, (off, n, shape) in self.layout.items():
            for flat in (self.m, self.v):
                a = flat[off:off + n].reshape(shape)
                flat[off:off + n] = self._state_from_reference(name, self._state_to_reference(name, a)).reshape(-1)


SMALL = Dims(H=3, W=4, D=16, map_dim=8, embed_dim_txt=6, embed_dim_nmn=5, lstm_dim=8, num_vocab_txt=11,
             num_choices=4, T_encoder=5, T_decoder=4, N=2)
SMALL_VQA = VQADims(H=2, W=2, D=14, map_dim=8, embed_dim_txt=6, embed_dim_nmn=5, lstm_dim=5, num_vocab_txt=9,
                    num_choices=7, T_encoder=4, T_decoder=3, N=2, qpn_hidden=4)


# ---- names ----------------------------------------------------------------------------------------------------------
def _expected_keys(names):
    want = []
    for n in names:
        want += [n + '/Adam', n + '/Adam_1']
    return want + ['beta1_power', 'beta2_power', 'n2nmn_amd/adam_step', 'n2nmn_amd/dropout_offset']


def test_key_set_clevr():
    names = list(variable_shapes(Dims()))
    keys = T.optimizer_state_keys(names)
    assert keys == _expected_keys(names) and len(set(keys)) == 2 * len(names) + 4
    assert 'baseline' not in keys
    tr = HostTrainer(variable_shapes(SMALL))
    st = tr.optimizer_state()
    assert list(st) == T.optimizer_state_keys(list(variable_shapes(SMALL)))
    for n, s in variable_shapes(SMALL).items():
        assert st[n + '/Adam'].shape == tuple(s) and st[n + '/Adam_1'].dtype == np.float32


def test_key_set_vqa_is_reference_shaped():
    names = list(vqa_variable_shapes(VQADims()))
    assert T.optimizer_state_keys(names) == _expected_keys(names)
    tr = HostVQATrainer(SMALL_VQA)
    st = tr.optimizer_state()
    ref = vqa_variable_shapes(SMALL_VQA)
    assert list(st) == _expected_keys(list(ref))
    padded = 0
    for n, s in ref.items():
        assert st[n + '/Adam'].shape == tuple(s) and st[n + '/Adam_1'].shape == tuple(s), n
        padded += tr.layout[n][2] != tuple(s)
    assert padded >= 10                # lstm_dim 5 -> 128 and D + 2 = 16 stay / pad: most variables are padded


def test_key_set_shapes_uses_reference_names():
    d = shapes_dims(num_vocab_txt=12, N=4)
    eng = shapes_engine_variable_shapes(d)
    names = [reference_name(k) for k in eng]
    assert any(a != b for a, b in zip(names, eng))
    assert T.optimizer_state_keys(names) == _expected_keys(names)
    tr = HostShapesTrainer({k: s for k, s in list(eng.items())})
    assert list(tr.optimizer_state()) == _expected_keys(names)
    assert any('layout_execution/AnswerModule/AnswerModule/' in k for k in tr.optimizer_state())


# ---- the step count ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iteration', [0, 1, 10, 899, 5000, 80000])
def test_step_recovered_from_beta_powers(iteration):
    """closed-form powers as optimizer_state() stores them, and the float32 running product TensorFlow keeps
    (the variable starts at beta and is multiplied by beta after every step): exact up to 5000; at 80000 within
    the drift bound derived in iteration_from_state's docstring (step_drift_bound: 5 steps)."""
    b1p, b2p = T.beta_powers(iteration, 0.9, 0.999)
    assert b1p.dtype == np.float32 and b2p.dtype == np.float32 and b2p.shape == ()
    assert b2p == np.float32(float(np.float32(0.999)) ** (iteration + 1))
    assert T.iteration_from_state({'beta1_power': b1p, 'beta2_power': b2p}, 0.999) == iteration
    beta = np.float32(0.999)
    prod = beta
    for _ in range(iteration):
        prod = np.float32(prod * beta)
    got = T.iteration_from_state({'beta1_power': np.float32(0), 'beta2_power': prod}, 0.999)
    bound = T.step_drift_bound(iteration, 0.999)
    assert bound == (0 if iteration <= 5000 else 5)
    print('iteration %d: float32 product gives %d (bound %d)' % (iteration, got, bound))
    assert abs(got - iteration) <= bound
    if iteration >= 899:
        assert T.beta_powers(iteration, 0.9, 0.999)[0] < 1e-38        # why beta1_power is not used


def test_drift_at_80000_does_not_change_the_update():
    """sqrt(1 - b2^t) / (1 - b1^t) at 80000 +- 5 steps is 1 to float32 resolution"""
    f = [np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t) for t in (79995, 80000, 80005)]
    assert all(np.float32(x) == np.float32(1.0) for x in f)


def test_explicit_adam_step_is_preferred():
    b1p, b2p = T.beta_powers(40, 0.9, 0.999)
    st = {'beta1_power': b1p, 'beta2_power': b2p, T.ADAM_STEP_KEY: np.int64(7)}
    assert T.iteration_from_state(st, 0.999) == 7
    with pytest.raises(KeyError):
        T.iteration_from_state({}, 0.999)


# ---- round trip on the host -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['clevr', 'vqa', 'shapes'])
def test_state_round_trip(kind):
    def make():
        if kind == 'vqa':
            return HostVQATrainer(SMALL_VQA)
        if kind == 'shapes':
            return HostShapesTrainer(shapes_engine_variable_shapes(shapes_dims(num_vocab_txt=12, N=4, lstm_dim=8,
                                                                               embed_dim=6, map_dim=8)))
        return HostTrainer(variable_shapes(SMALL))
    a, b = make(), make()
    a.fill(seed=1, iteration=3, offset=12345)
    st = a.optimizer_state()
    assert int(st[T.ADAM_STEP_KEY]) == 3 and st[T.ADAM_STEP_KEY].dtype in tf_checkpoint._DTYPE_CODES
    b.load_optimizer_state(st)
    assert b.iteration == 3 and b.dropout_stream.offset == 12345
    assert np.array_equal(a.m, b.m) and np.array_equal(a.v, b.v)
    back = b.optimizer_state()
    assert list(back) == list(st) and all(np.array_equal(back[k], st[k]) for k in st)


def test_load_strictness_and_shape_errors():
    tr = HostTrainer(variable_shapes(SMALL))
    tr.fill(seed=2, iteration=5)
    st = tr.optimizer_state()
    name = next(n for n, s in variable_shapes(SMALL).items() if len(s) == 2)
    partial = {k: v for k, v in st.items() if not k.startswith(name + '/Adam')}
    other = HostTrainer(variable_shapes(SMALL))
    with pytest.raises(KeyError):
        other.load_optimizer_state(partial)
    other.load_optimizer_state(partial, strict=False)
    off, n, _ = other.layout[name]
    assert not other.m[off:off + n].any() and not other.v[off:off + n].any()
    rest = np.ones(other.numel, bool)
    rest[off:off + n] = False
    assert np.array_equal(other.m[rest], tr.m[rest]) and other.iteration == 5
    bad = dict(st)
    bad[name + '/Adam_1'] = st[name + '/Adam_1'].T.copy()
    with pytest.raises(ValueError, match=re.escape(name)):
        HostTrainer(variable_shapes(SMALL)).load_optimizer_state(bad)
    one = {k: v for k, v in st.items() if k != name + '/Adam_1'}
    with pytest.raises(KeyError):
        HostTrainer(variable_shapes(SMALL)).load_optimizer_state(one, strict=False)


# ---- the Saver ---------------------------------------------------------------------------------------------------------
class StubModel:
    """what the Saver asks of a model face"""

    def __init__(self, shapes, seed=0):
        rng = np.random.default_rng(seed)
        self.shapes = dict(shapes)
        self.w = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
        self.loaded = None

    def variable_shapes(self):
        return self.shapes

    def get_weights(self):
        return dict(self.w)

    def load_weights(self, weights):
        unknown = set(weights) - set(self.shapes)
        assert not unknown, unknown               # (the engine refuses names that are not its variables)
        self.loaded = dict(weights)
        self.w.update({k: np.array(v) for k, v in weights.items()})


@pytest.fixture
def stub(monkeypatch):
    model = StubModel(variable_shapes(SMALL))
    monkeypatch.setattr(runtime, '_MODELS', [model])
    monkeypatch.setattr(runtime_train, '_GLOBALS', [])
    monkeypatch.setattr(runtime, '_SAVE_OPTIMIZER_STATE', [False])
    trainer = HostTrainer(variable_shapes(SMALL))
    trainer.fill(seed=3, iteration=3, offset=77)
    return model, trainer


def test_saver_default_output_is_unchanged(stub, tmp_path):
    model, trainer = stub
    runtime.attach_trainer(model, trainer)
    path = runtime.tf.train.Saver().save(None, str(tmp_path / 'snap'))
    back = tf_checkpoint.read_checkpoint(path)
    assert set(back) == set(model.shapes)
    runtime.tf.train.Saver().restore(None, path)
    assert set(model.loaded) == set(model.shapes)              # a file without slots: every entry to load_weights


def test_saver_writes_and_restores_the_state_with_the_switch_on(stub, tmp_path):
    model, trainer = stub
    runtime.attach_trainer(model, trainer)
    assert runtime.save_optimizer_state(True) is False
    path = runtime.tf.train.Saver().save(None, str(tmp_path / 'snap'), global_step=3)
    assert path.endswith('snap-3')
    back = tf_checkpoint.read_checkpoint(path)
    st = trainer.optimizer_state()
    assert set(back) == set(model.shapes) | set(st) and len(st) == 2 * len(model.shapes) + 4
    for k, v in st.items():
        assert back[k].dtype == np.asarray(v).dtype and back[k].shape == np.asarray(v).shape, k
        assert back[k].tobytes() == np.asarray(v).tobytes(), k
    # restore into an existing trainer, through a var_list that names the model's variables only
    other = HostTrainer(variable_shapes(SMALL))
    runtime.attach_trainer(model, other)
    runtime.tf.train.Saver(runtime_train.model_variables(model)).restore(None, path)
    assert set(model.loaded) == set(model.shapes)
    assert np.array_equal(other.m, trainer.m) and np.array_equal(other.v, trainer.v)
    assert other.iteration == 3 and other.dropout_stream.offset == 77
    assert runtime.save_optimizer_state(False) is True


def test_saver_var_list_passes_slots_with_their_variable(stub, tmp_path):
    model, trainer = stub
    runtime.attach_trainer(model, trainer)
    runtime.save_optimizer_state(True)
    some = runtime_train.model_variables(model)[:3]
    path = runtime.tf.train.Saver(some).save(None, str(tmp_path / 'part'))
    back = tf_checkpoint.read_checkpoint(path)
    want = set()
    for v in some:
        want |= {v.name, v.name + '/Adam', v.name + '/Adam_1'}
    assert set(back) == want | {'beta1_power', 'beta2_power', T.ADAM_STEP_KEY, T.DROPOUT_OFFSET_KEY}


def test_restore_before_the_trainer_exists_reaches_it_when_it_is_created(stub, tmp_path, monkeypatch):
    model, trainer = stub
    runtime.attach_trainer(model, trainer)
    runtime.save_optimizer_state(True)
    path = runtime.tf.train.Saver().save(None, str(tmp_path / 'snap'))
    # a new process: same model, no trainer yet
    fresh = StubModel(variable_shapes(SMALL), seed=9)
    monkeypatch.setattr(runtime, '_MODELS', [fresh])
    runtime.tf.train.Saver().restore(None, path)
    assert all(np.array_equal(fresh.w[k], model.w[k]) for k in model.w)
    assert getattr(fresh, '_trainer', None) is None and fresh._pending_optimizer_state
    # the first fetched train_step creates the trainer (TrainStep.ensure_trainer): a constructor that resets
    made = []

    def new_trainer(m, plan, op):
        made.append(HostTrainer(variable_shapes(SMALL)))
        return made[-1]
    monkeypatch.setattr(runtime_train, '_new_trainer', new_trainer)
    step = object.__new__(runtime_train.TrainStep)
    step.trainer, step.model, step.op = None, fresh, None
    step.plan = types.SimpleNamespace(objective=0)
    tr = step.ensure_trainer()
    assert tr is made[0] and fresh._trainer is tr and not fresh._pending_optimizer_state
    assert np.array_equal(tr.m, trainer.m) and np.array_equal(tr.v, trainer.v)
    assert tr.iteration == 3 and tr.dropout_stream.offset == 77
    assert step.ensure_trainer() is tr and len(made) == 1
