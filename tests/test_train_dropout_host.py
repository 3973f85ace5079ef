"""Dropout and the training step, host side (no GPU): the CLEVR training step has no LSTM dropout, so a
train_step fetched from a CLEVR model built with encoder_dropout / decoder_dropout is refused instead of
sampling under dropout masks and differentiating without them.  The model runs over the CPU oracle
(tests/oracle_engine.py)."""
import types

import pytest

from n2nmn_amd import runtime, runtime_train, train
from n2nmn_amd.nmn3_assembler import Assembler
from n2nmn_amd.nmn3_model import NMN3Model
from n2nmn_amd.spec import CLEVR_MODULE_NAMES, Dims
from oracle_engine import OracleEngine, OracleTrainer


def _model(monkeypatch, encoder_dropout, decoder_dropout):
    monkeypatch.setattr(runtime, '_MODELS', [])
    d = Dims(N=4)
    asm = Assembler(list(CLEVR_MODULE_NAMES))
    feat = runtime.placeholder('float32', [None, d.H, d.W, d.D])
    seq = runtime.placeholder('int32', [None, None])
    lens = runtime.placeholder('int32', [None])
    return NMN3Model(feat, seq, lens, T_decoder=d.T_decoder, num_vocab_txt=d.num_vocab_txt,
                     embed_dim_txt=d.embed_dim_txt, num_vocab_nmn=d.num_vocab_nmn, embed_dim_nmn=d.embed_dim_nmn,
                     lstm_dim=d.lstm_dim, num_layers=d.num_layers, assembler=asm,
                     encoder_dropout=encoder_dropout, decoder_dropout=decoder_dropout, decoder_sampling=False,
                     num_choices=d.num_choices, engine=OracleEngine(d, asm))


def _plan_and_op():
    plan = types.SimpleNamespace(weight_decay=5e-6)
    op = types.SimpleNamespace(optimizer=types.SimpleNamespace(hyper=dict(lr=1e-3, beta1=0.9, beta2=0.999,
                                                                          eps=1e-8)),
                               clip_norm=10.0)
    return plan, op


@pytest.mark.parametrize('enc,dec', [(True, False), (False, True), (True, True)])
def test_clevr_train_step_refuses_lstm_dropout(monkeypatch, enc, dec):
    monkeypatch.setattr(train, 'Trainer', OracleTrainer)
    model = _model(monkeypatch, enc, dec)
    with pytest.raises(NotImplementedError, match='dropout'):
        runtime_train._new_trainer(model, *_plan_and_op())


def test_clevr_train_step_without_dropout_builds_the_plain_trainer(monkeypatch):
    monkeypatch.setattr(train, 'Trainer', OracleTrainer)
    model = _model(monkeypatch, False, False)
    tr = runtime_train._new_trainer(model, *_plan_and_op())
    assert type(tr) is OracleTrainer and tr.engine is model.engine
    assert tr.weight_decay == 5e-6 and tr.hyper['max_grad_l2_norm'] == 10.0
