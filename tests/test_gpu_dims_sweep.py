"""The dimension space n2nmn_ctx_create accepts, point by point (tests/dims_points.py), against the fp64
oracles: one engine (and one Trainer) per point, every stage of the model at 9 and at 130 rows.  130 rows
switch on the throughput routes (lstm_tile / the wide step, several decoder steps per attention workgroup,
the chip-wide walker front end, deferred pooling, the staged walker).

Bars (none of them new: tests/test_gpu_kernels.py::test_attention_extremes, tests/test_gpu_train.py,
tests/test_gpu_walker.py):
  forward    |got - want| <= 1e-4 * max(1, max|want|)
  gradients  2e-4 * max|want| + 1e-7 per tensor, through test_gpu_train._check (selection-gap protocol)
  walker against the level path   2e-5
A context the library accepts computes what the oracle computes; what it cannot compute it refuses with a
message that names the field.  profiles/dims_sweep.md records the route and the largest error per point.
"""
import ctypes as C

import numpy as np
import pytest

import dims_points as DP
from oracle import n2nmn_oracle as O
from util import greedy_tokens_under_margin_rule, maxdiff, t2n
from test_gpu_kernels import ALL_OPS, _oracle_module, _rand_case
from test_gpu_train import WD, _check

pytestmark = pytest.mark.gpu
NAMES = DP.NAMES
FWD_TOL = 1e-4
PATH_TOL = 2e-5          # walker against the level path
SMALL, LARGE = DP.BATCH_SIZES
F_WALK, F_SCHED, F_POOL, F_TMAP, F_FIND = 'walk(layout walker)', 'sched(', 'pool', 'walk_tmap(', 'walk_find('


def fwd_close(what, got, want):
    """the forward bar; prints the figure before it asserts"""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    d = maxdiff(got, want)
    print('%-58s max|diff| %.3e  bar %.3e' % (what, d, FWD_TOL * scale))
    assert np.isfinite(got).all(), what + ': non-finite values'
    assert d <= FWD_TOL * scale, '%s: max |diff| = %.3e > %.3e' % (what, d, FWD_TOL * scale)
    return d


class PointState:
    def __init__(self, p):
        from n2nmn_amd.engine import Engine
        from n2nmn_amd.nmn3_assembler import Assembler
        self.p, self.d = p, p.dims
        self.asm = Assembler(NAMES)
        self.eng = Engine(p.dims, self.asm)
        self.w = DP.weights(p)
        self.eng.load_weights(self.w)
        self._ref, self._trainer = {}, {}

    def ref(self, n):
        """fp64 forward of the point's batch of n under its layouts, computed once"""
        if n not in self._ref:
            batch, toks = DP.inputs(self.p, n), DP.layouts(self.p, n)
            r = O.forward(self.w, NAMES, batch, self.d.T_decoder, self.d.num_choices, np.float64,
                          use_gt_layout=True, gt_layout=toks)
            assert r['validity'].all()
            self._ref[n] = (batch, toks, r)
        return self._ref[n]

    def mode(self, n):
        self.eng.set_mode('throughput' if n >= 128 else 'latency')

    def families(self, fn):
        """run fn() under the profiler -> (fn's result, {family name: launches}, walk stats)"""
        from n2nmn_amd import _lib
        self.eng.profile_begin()
        out = fn()
        fams = {f['name']: f['launches'] for f in self.eng.profile_end()}
        st = (C.c_uint64 * 10)()
        _lib.check(self.eng._lib.n2nmn_debug_walk_stats(self.eng._ctx, st))
        return out, fams, [int(x) for x in st]


def _fam(fams, prefix):
    hit = [v for k, v in fams.items() if k.startswith(prefix)]
    assert len(hit) == 1, (prefix, sorted(fams))
    return hit[0]


@pytest.fixture(scope='module', params=DP.ACCEPTED, ids=lambda p: p.name)
def pt(request):
    st = PointState(request.param)
    yield st
    st.eng.set_mode('latency')


def test_walker_support_is_what_the_table_states(pt):
    assert pt.eng.walk_supported() == pt.p.walker, pt.p.why


@pytest.mark.parametrize('n', DP.BATCH_SIZES)
def test_seq2seq_teacher_forced(pt, n):
    """encoder outputs and final states, token_scores, word_vecs, attention, token_probs"""
    batch, toks, ref = pt.ref(n)
    pt.mode(n)
    out = pt.eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], use_gt_layout=True,
                         gt_layout=toks, debug=True)
    enc, dec = ref['enc'], ref['dec']
    tag = '%s N=%d ' % (pt.p.name, n)
    assert np.array_equal(t2n(out['predicted_tokens']), toks)
    fwd_close(tag + 'encoder_outputs', t2n(out['encoder_outputs']), enc['outputs'])
    fwd_close(tag + 'encoder_h_transformed', t2n(out['encoder_h_transformed']), enc['h_transformed'])
    st = t2n(out['encoder_states'])
    for l in range(2):
        fwd_close(tag + 'c%d' % l, st[l, 0], enc['states'][l][0])
        fwd_close(tag + 'h%d' % l, st[l, 1], enc['states'][l][1])
    fwd_close(tag + 'token_scores', t2n(out['token_scores']), dec['token_scores'])
    fwd_close(tag + 'atts', t2n(out['atts']), dec['atts'][..., 0])
    fwd_close(tag + 'word_vecs', t2n(out['word_vecs']), dec['word_vecs'])
    fwd_close(tag + 'token_probs', t2n(out['token_probs']), dec['token_probs'])
    atts = t2n(out['atts'])
    lens = batch['seq_length_batch']
    past = np.arange(pt.d.T_encoder)[None, :, None] >= lens[None, None, :]
    assert np.all(atts[np.broadcast_to(past, atts.shape)] == 0.0)


def test_greedy_decoding_one_step_per_launch(pt):
    batch, toks, ref = pt.ref(SMALL)
    pt.mode(SMALL)
    asm = pt.asm
    dec = O.decoder_forward(pt.w, ref['enc'], asm.P, asm.W, asm.b, pt.d.T_decoder, np.float64)
    out = pt.eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'])
    tok = t2n(out['predicted_tokens'])
    _, validity = asm.assemble_packed(tok)
    assert validity.all()
    flipped = greedy_tokens_under_margin_rule(tok, dec, pt.p.name)
    print('%s: %d of %d greedy layouts differ at a near-tie' % (pt.p.name, len(flipped), SMALL))
    # the oracle's tokens forced through the same one-step launches: every per-step quantity comparable
    out = pt.eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], debug=True,
                         forced_tokens=dec['predicted_tokens'])
    tag = pt.p.name + ' greedy '
    fwd_close(tag + 'token_scores', t2n(out['token_scores']), dec['token_scores'])
    fwd_close(tag + 'atts', t2n(out['atts']), dec['atts'][..., 0])
    fwd_close(tag + 'word_vecs', t2n(out['word_vecs']), dec['word_vecs'])
    fwd_close(tag + 'token_probs', t2n(out['token_probs']), dec['token_probs'])


def _phase1(pt, batch, toks):
    return pt.eng.seq2seq(batch['input_seq_batch'], batch['seq_length_batch'], forced_tokens=toks,
                          reuse_buffers=False)


@pytest.mark.parametrize('n', DP.BATCH_SIZES)
def test_execution_level_path_and_walker(pt, n):
    """the level path (host assembler + n2nmn_execute_program), n2nmn_execute_tokens as the context routes it,
    and -- where the walker serves the point -- every combination of its three switches"""
    batch, toks, ref = pt.ref(n)
    pt.mode(n)
    eng, asm, p = pt.eng, pt.asm, pt.p
    tag = '%s N=%d ' % (p.name, n)
    s2s = _phase1(pt, batch, toks)
    feat = batch['image_feat_batch']
    packed, v = asm.assemble_packed(toks)
    assert v.all()
    lvl = t2n(eng.execute(packed, feat, s2s['word_vecs'])).copy()
    fwd_close(tag + 'level path', lvl, ref['scores'])
    table = (s2s['atts'], s2s['_input_seq'], s2s['_seq_length'])

    def default_route():
        sc, val = eng.execute_tokens(s2s['predicted_tokens'], feat, s2s['word_vecs'], reuse_buffers=False,
                                     atts=table if p.walker else None)
        return t2n(sc).copy(), t2n(val).copy()
    (got, val), fams, stats = pt.families(default_route)
    assert val.all()
    fwd_close(tag + 'execute_tokens', got, ref['scores'])
    if not p.walker:
        # the fallback: assembled and scheduled on the device, no walker launch
        assert _fam(fams, F_SCHED) >= 1 and _fam(fams, F_WALK) == 0, fams
        assert maxdiff(got, lvl) <= PATH_TOL
        return
    assert _fam(fams, F_WALK) >= 1 and _fam(fams, F_SCHED) == 0, fams
    assert stats[5] == n                                   # every question counted once, as valid
    roots = toks[(toks != asm.EOS_idx).sum(0) - 1, np.arange(n)]
    pooled_roots = int(np.isin(roots, [asm.name2idx_dict['_Describe'], asm.name2idx_dict['_SameProperty']]).sum())
    assert pooled_roots >= 2
    if n >= 128:
        # the chip-wide front end ran; the pooling roots left the walker exactly where walk_pool_kernel exists
        assert _fam(fams, F_TMAP) >= 1 and _fam(fams, F_FIND) >= 1, fams
        assert stats[6] == (pooled_roots if p.defer_pool else 0), (stats, pooled_roots)
        assert (_fam(fams, F_POOL) >= 1) == p.defer_pool, fams
    else:
        assert _fam(fams, F_TMAP) == 0 and _fam(fams, F_POOL) == 0 and stats[6] == 0, (fams, stats)
    print(tag + 'walker vs level path %.3e' % maxdiff(got, lvl))
    assert maxdiff(got, lvl) <= PATH_TOL
    # word_vecs instead of the attention tables (walk_textmap_kernel)
    sc, val = eng.execute_tokens(s2s['predicted_tokens'], feat, s2s['word_vecs'], reuse_buffers=False)
    assert t2n(val).all()
    fwd_close(tag + 'walker fed with word_vecs', t2n(sc), ref['scores'])
    assert maxdiff(t2n(sc), lvl) <= PATH_TOL
    worst = 0.0
    try:
        for staged in (0, 1):
            for defer in (0, 1):
                for front in (0, 1):
                    eng.set_staged(staged); eng.set_defer_pool(defer); eng.set_front_end(front)
                    sc, val = eng.execute_tokens(s2s['predicted_tokens'], feat, None, reuse_buffers=False,
                                                 atts=table)
                    what = tag + 'walker staged=%d defer_pool=%d front_end=%d' % (staged, defer, front)
                    assert t2n(val).all(), what
                    fwd_close(what, t2n(sc), ref['scores'])
                    dl = maxdiff(t2n(sc), lvl)
                    worst = max(worst, dl)
                    assert dl <= PATH_TOL, '%s: differs from the level path by %.3e' % (what, dl)
    finally:
        eng.set_staged(-1); eng.set_defer_pool(-1); eng.set_front_end(-1)
    print(tag + 'worst walker setting vs level path %.3e' % worst)


def test_invalid_layouts_get_the_oracles_validity_and_zero_rows(pt):
    n = SMALL
    batch = DP.inputs(pt.p, n)
    toks = DP.invalid_layouts(pt.p, n)
    pt.mode(n)
    eng = pt.eng
    ref = O.forward(pt.w, NAMES, batch, pt.d.T_decoder, pt.d.num_choices, np.float64, forced_tokens=toks)
    bad = list(DP.INVALID_COLUMNS)
    assert not ref['validity'][bad].any() and ref['validity'].sum() == n - len(bad)
    s2s = _phase1(pt, batch, toks)
    table = (s2s['atts'], s2s['_input_seq'], s2s['_seq_length'])
    settings = [(-1, -1, -1)] + ([(1, 1, 1), (0, 1, 1)] if pt.p.walker else [])
    try:
        for staged, defer, front in settings:
            eng.set_staged(staged); eng.set_defer_pool(defer); eng.set_front_end(front)
            sc, val = eng.execute_tokens(s2s['predicted_tokens'], batch['image_feat_batch'], s2s['word_vecs'],
                                         reuse_buffers=False, atts=table if pt.p.walker else None)
            sc, val = t2n(sc), t2n(val).astype(bool)
            assert np.array_equal(val, ref['validity']), (staged, defer, front)
            assert np.all(sc[bad] == 0.0)
            fwd_close('%s invalid mix %s' % (pt.p.name, (staged, defer, front)), sc, ref['scores'])
    finally:
        eng.set_staged(-1); eng.set_defer_pool(-1); eng.set_front_end(-1)


def test_every_operator_through_module_forward(pt):
    d = pt.d
    small = DP.with_n(pt.p, 8)                # 8 images are enough for explicit inputs
    for name in ALL_OPS:
        for nb in (1, 7):
            rng = np.random.default_rng(ALL_OPS.index(name) * 100 + nb)
            feat, wv, t_idx, b_idx, a0, a1 = _rand_case(small, rng, nb)
            from n2nmn_amd.spec import MODULE_INPUT_NUM
            ins = [a0, a1][:MODULE_INPUT_NUM[name]]
            got = t2n(pt.eng.module_forward(name, ins, t_idx, b_idx, feat, wv))
            want = _oracle_module(pt.w, name, feat, wv, t_idx, b_idx, a0, a1, d)
            fwd_close('%s %s nb=%d' % (pt.p.name, name, nb), got, want)


def _trainer(pt, n):
    """one Trainer per point; a training batch of >= 128 rows runs in throughput mode"""
    from n2nmn_amd.train import Trainer
    pt.mode(n)
    if 'tr' not in pt._trainer:
        pt._trainer['tr'] = Trainer(pt.eng, weight_decay=WD)
    return pt._trainer['tr']


@pytest.mark.parametrize('n', DP.BATCH_SIZES)
def test_training_step_against_the_autograd_oracle(pt, n):
    """losses, scores, the five intermediate gradients and every variable's gradient (test_gpu_train._check);
    where n2nmn_train_enable must refuse, its outcome instead"""
    p = pt.p
    if p.train is not None:
        from n2nmn_amd.train import Trainer
        with pytest.raises(ValueError) as e:
            Trainer(pt.eng, weight_decay=WD)
        assert 'train_enable' in str(e.value) and p.train in str(e.value), str(e.value)
        return
    tr = _trainer(pt, n)
    if p.forward_only:                        # C = 1: the loss is constant; train_enable's outcome only
        assert tr.numel > 0
        return
    batch, toks, _ = pt.ref(n)
    rows = _check(tr, pt.d, pt.w, batch, toks, clear_examples_only=True)
    worst = max(rows, key=lambda r: r[2] / (2e-4 * r[1] + 1e-7))
    print('%s N=%d worst gradient: %s diff %.3e at scale %.3e (%.2f of the bar)' %
          (p.name, n, worst[0][-60:], worst[2], worst[1], worst[2] / (2e-4 * worst[1] + 1e-7)))


# ---- refusals: N2NMN_EINVAL / N2NMN_ECAPACITY and a message that names the field -------------------------
def _create(**kw):
    """n2nmn_ctx_create on the dims of `m64` (capacity 4) with fields replaced -> (return code, message)"""
    import dataclasses
    from n2nmn_amd import _lib
    d = dataclasses.replace(DP.BY_NAME['m64'].dims, N=4, **kw)
    L = _lib.lib()
    cd = _lib.Dims(**{k: int(v) for k, v in d.asdict().items()})
    ctx = C.c_void_p()
    rc = L.n2nmn_ctx_create(C.byref(cd), 0, C.byref(ctx))
    msg = L.n2nmn_last_error().decode() if rc != 0 else ''
    if rc == 0:
        L.n2nmn_ctx_destroy(ctx)
    return rc, msg


REFUSED = [
    (dict(lstm_dim=1152), 'lstm_dim'),              # the point `l1152`
    (dict(lstm_dim=2048), 'lstm_dim'),
    (dict(lstm_dim=192), 'lstm_dim'),
    (dict(map_dim=1025), 'map_dim'),
    (dict(D=24), 'D must'),
    (dict(D=4112), 'D must'),
    (dict(embed_dim_txt=6, embed_dim_nmn=6), 'embed'),
    (dict(embed_dim_txt=100, embed_dim_nmn=104), 'embed'),
    (dict(kernel_size=7), 'kernel_size'),
    (dict(num_vocab_nmn=17), 'num_vocab_nmn'),
    (dict(num_layers=3), 'num_layers'),
    (dict(T_encoder=60, embed_dim_txt=300, embed_dim_nmn=300), 'T_encoder'),
    (dict(num_choices=0), 'num_choices'),
    (dict(D=0), 'D must'),
    (dict(embed_dim_txt=0, embed_dim_nmn=0), 'embed_dim_txt'),
    (dict(H=0), 'H must'),
]


@pytest.mark.parametrize('fields,word', REFUSED, ids=[w + '-' + '-'.join('%s' % v for v in f.values())
                                                      for f, w in REFUSED])
def test_ctx_create_refuses_with_a_message_that_names_the_field(fields, word):
    rc, msg = _create(**fields)
    assert rc in (-1, -4), (rc, msg)                # N2NMN_EINVAL / N2NMN_ECAPACITY
    assert msg.startswith('ctx_create') and word in msg, msg


def test_the_refused_point_of_the_table():
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    for p in DP.POINTS:
        if p.refused is None:
            continue
        with pytest.raises(ValueError) as e:
            Engine(p.dims, Assembler(NAMES))
        assert p.refused in str(e.value), str(e.value)
    # the largest lstm_dim is accepted
    rc, msg = _create(lstm_dim=1024)
    assert rc == 0, msg


def test_calls_beyond_a_contexts_capacity_are_refused():
    """N, T_encoder, T_decoder above what the context was created for: N2NMN_ECAPACITY (ValueError), the
    message names the call"""
    import dataclasses
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    p = DP.BY_NAME['m64']
    d = dataclasses.replace(p.dims, N=4)
    eng = Engine(d, Assembler(NAMES))
    eng.load_weights(DP.weights(p))
    b = DP.inputs(p, 9)
    with pytest.raises(ValueError):
        eng.seq2seq(b['input_seq_batch'], b['seq_length_batch'])
    b4 = DP.inputs(p, 4)
    with pytest.raises(ValueError):
        eng.seq2seq(b4['input_seq_batch'], b4['seq_length_batch'], T_dec=d.T_decoder + 1)
