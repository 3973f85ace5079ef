"""Dimension points of the CLEVR variant that n2nmn_ctx_create accepts (or must refuse), one per kernel
route or padding edge of the host dispatch, with the inputs every point is tested on.  Plain data and
helpers for tests/test_dims_points_host.py (fp64 oracles only) and tests/test_gpu_dims_sweep.py.

Every point keeps T_encoder = 11 and T_decoder = 10, so an oracle call stays cheap and
T_encoder * embed_dim + T_decoder * T_encoder <= 16000 (n2nmn_ctx_create) holds everywhere.

Route notes name the host dispatch they come from: Mp = round_up(map_dim, 64) and HWp = round_up(H * W, 32)
(capi.cpp), launch_walk_find / launch_walk / walk_supported / walk_pool_supported (kernels_walk.hip),
launch_dec_attn / launch_lstm_step (kernels_seq2seq.hip), n2nmn_train_enable (capi_train.cpp).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from n2nmn_amd import synth
from n2nmn_amd.spec import CLEVR_MODULE_NAMES, Dims
from oracle import n2nmn_oracle as O

NAMES = list(CLEVR_MODULE_NAMES)
T_ENC, T_DEC = 11, 10
BATCH_SIZES = (9, 130)           # 130 >= 128: lstm_tile / the wide step, per-question decoder attention,
N_CAP = max(BATCH_SIZES)         # chip-wide walker front end, deferred pooling


class Point(NamedTuple):
    name: str
    dims: Dims
    walker: Optional[bool]       # n2nmn_walk_supported expected (None: the context is refused)
    train: Optional[str]         # None: n2nmn_train_enable succeeds; else a word of its refusal message
    refused: Optional[str]       # None: n2nmn_ctx_create succeeds; else a word of its refusal message
    forward_only: bool
    why: str
    defer_pool: bool = True      # walk_pool_supported expected (only read where the walker is)


def _d(H, W, D, M, E, L, C, ks):
    return Dims(H=H, W=W, D=D, map_dim=M, embed_dim_txt=E, embed_dim_nmn=E, lstm_dim=L, num_choices=C,
                kernel_size=ks, num_vocab_nmn=15, T_encoder=T_ENC, T_decoder=T_DEC, N=N_CAP)


POINTS: List[Point] = [
    Point('floor', _d(1, 1, 16, 1, 4, 128, 1, 3), True, None, None, True,
          'the minimum of every field; C = 1 makes the loss constant, so forward and the outcome of '
          'train_enable only', defer_pool=False),
    Point('m64', _d(4, 8, 64, 64, 100, 128, 33, 5), True, None, None, False,
          'Mp == map_dim, HWp == H*W: no padding anywhere; walk_find16<1>; lstm 128: dec_attn_kernel<256>, '
          'two 64-column LSTM tiles'),
    Point('m65', _d(3, 11, 48, 65, 36, 384, 2, 3), False, None, None, False,
          '63 padded columns, 31 padded pixels; D/4 = 12 does not divide 512: no walker, execute_tokens '
          'through the level path; lstm 384: dec_attn_kernel<256> with a ragged last column group'),
    Point('m128', _d(5, 7, 32, 100, 52, 128, 10, 3), True, None, None, False,
          'Mp 128 with a walker (m65 has none): walk_find16<2>; 28 padded columns, 29 padded pixels; kernel 3 '
          'in the walker\'s Transform'),
    Point('m129', _d(8, 8, 128, 129, 300, 256, 500, 5), True, None, None, False,
          'Mp 192: walk_find16<3>; C near the walker\'s 512; map_dim * C = 64500 just under the fused head\'s 65536'),
    Point('m257', _d(13, 14, 256, 257, 300, 640, 7, 5), True, None, None, False,
          'Mp 320: walk_find_kernel<2,false>, walk_kernel<2>; H*W 182 just under 192 (three pixel groups)'),
    Point('m577', _d(2, 19, 2048, 577, 300, 768, 100, 5), True, None, None, False,
          'Mp 640: the <4> instantiations; D/4 = 512: one feature row per thread, H*W = 38 = WALK_POOL_ROWS; '
          'lstm 768: dec_attn_multi<4,*>'),
    Point('m1024', _d(1, 5, 32, 1024, 200, 1024, 64, 5), True, None, None, False,
          'map_dim and lstm_dim at their limits; map_dim * C == 65536 exactly: still the fused head'),
    # walk_pool_kernel's row count is a quarter of the walker's (256 threads over D/32 columns against 512 over
    # D/4), so the walker's 38 rows always imply the pool kernel's 10: the only dimensions with a walker and
    # without walk_pool_supported are D = 16 (D % 32 != 0)
    Point('hw161', _d(7, 23, 16, 250, 300, 128, 28, 5), True, None, None, False,
          'walker supported, walk_pool_supported false (D = 16 has no 8 channel parts of 4): at K*N >= 128 the '
          'deferred pooling must fall back to inline pooling; 31 padded pixels', defer_pool=False),
    Point('rows41', _d(7, 23, 512, 250, 300, 128, 28, 5), False, None, None, False,
          'H*W = 161 at D = 512 is 41 feature rows per walker thread, over WALK_POOL_ROWS = 38 (m577 sits on it): '
          'no walker, execute_tokens through the level path, training allowed'),
    Point('hw196', _d(14, 14, 64, 64, 100, 128, 4, 5), False, 'H*W', None, False,
          'H*W > 192 in the CLEVR variant: forward through the level path, train_enable refuses'),
    Point('bighead', _d(8, 8, 128, 129, 100, 128, 512, 5), False, 'map_dim', None, False,
          'map_dim * C > 65536 outside models_vqa: the split answer head forward, train_enable refuses'),
    Point('l1152', _d(2, 3, 64, 64, 100, 1152, 4, 3), None, None, 'lstm_dim', True,
          'lstm_dim above the four 256-column groups of the decoder attention kernels: refused'),
]
BY_NAME: Dict[str, Point] = {p.name: p for p in POINTS}
ACCEPTED = [p for p in POINTS if p.refused is None]
TRAINABLE = [p for p in ACCEPTED if p.train is None and not p.forward_only]

# layouts that random walks and the ten templates never produced at these sizes (_EqualNum, _LessNum,
# _SameProperty) plus one use of every other operator: together all 14
HAND_LAYOUTS = (
    ('_Scene', '_Filter', '_Exist'),
    ('_Find', '_Find', '_EqualNum'),
    # (Transform and FindSameProperty each feed a head without a spatial soft-max here: under _Describe /
    # _SameProperty alone the gradient of their conv_eltwise bias is exactly zero)
    ('_Find', '_FindSameProperty', '_Find', '_Transform', '_LessNum'),
    ('_Find', '_FindSameProperty', '_Find', '_SameProperty'),
    ('_Find', '_Find', '_Or', '_Find', '_And', '_Count'),
    ('_Find', '_Transform', '_Filter', '_Describe'),
    ('_Find', '_Find', '_MoreNum'),
)


def seed_of(p: Point) -> int:
    return 100 + [q.name for q in POINTS].index(p.name)


def weights(p: Point):
    return synth.make_weights(p.dims, seed=seed_of(p))


def inputs(p: Point, n: int):
    """synth.make_inputs(min_len=1) with question 0 forced to length 1 and question 1 to T_encoder"""
    d = p.dims
    b = synth.make_inputs(d, seed=seed_of(p) + n, n=n, min_len=1)
    lens = b['seq_length_batch']
    lens[0] = 1
    if n > 1:
        lens[1] = d.T_encoder
        b['input_seq_batch'][:, 1] = np.random.default_rng(seed_of(p)).integers(0, d.num_vocab_txt, d.T_encoder)
    seq = b['input_seq_batch']
    seq[np.arange(d.T_encoder)[:, None] >= lens[None, :]] = 0
    return b


def layouts(p: Point, n: int) -> np.ndarray:
    """[T_decoder, n] int32: the hand-written list first, then templates and random automaton walks by turns"""
    d = p.dims
    P, W, b = O.build_validity_mats(NAMES)
    rnd = synth.random_valid_layouts(d, P, W, b, seed=seed_of(p) + n, n=n, max_len=6)
    tpl = synth.template_layout_batch(d, n=n, offset=seed_of(p))
    out = np.zeros((d.T_decoder, n), np.int32)
    for i in range(n):
        if i < len(HAND_LAYOUTS):
            out[:, i] = synth.module_list2tokens(HAND_LAYOUTS[i], d.T_decoder)
        else:
            out[:, i] = tpl[:, i] if (i & 1) else rnd[:, i]
    return out


def invalid_layouts(p: Point, n: int) -> np.ndarray:
    """layouts(p, n) with the five kinds of invalid layout of test_walker_mixed_valid_and_invalid_rows in
    columns 0, 2, 3, 5 and 7"""
    idx = {s: i for i, s in enumerate(NAMES)}
    eos = idx['<eos>']
    toks = layouts(p, n).copy()
    assert n >= 8
    toks[:, 0] = eos                                              # empty layout
    toks[:, 2] = idx['_Find']                                     # no <eos>
    toks[:, 3] = eos
    toks[:3, 3] = [idx['_Find'], idx['_And'], idx['_Count']]      # not enough input for _And
    toks[:, 5] = eos
    toks[:3, 5] = [idx['_Find'], idx['_Count'], idx['_Exist']]    # ans fed to _Exist
    toks[:, 7] = eos
    toks[:2, 7] = [idx['_Find'], idx['_Transform']]               # result type must be ans
    return toks


INVALID_COLUMNS = (0, 2, 3, 5, 7)


def operators_used(toks: np.ndarray):
    return {NAMES[int(t)] for t in np.unique(toks)} - {'<eos>'}


def with_n(p: Point, n: int) -> Dims:
    return dataclasses.replace(p.dims, N=n)
