"""Compact feature feed, host half (n2nmn_amd/data_reader.py, n2nmn_amd/feed.py, include/n2nmn.h section 11):
the reader's `feature_dtype` / `dedupe_features` options, the binding of the two new entry points and the
index validation of Engine.features.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import data_reader_cases as DC  # noqa: E402

from n2nmn_amd import _lib, data_reader
from n2nmn_amd.data_reader import DataReader


def test_entry_points_are_bound_and_exported():
    bound = {s[0]: s for s in _lib.SYMBOLS}
    assert len(bound['n2nmn_features_expand'][2]) == 10 and len(bound['n2nmn_features_narrow'][2]) == 4
    L = ctypes.CDLL(_lib.lib_path()) if os.path.exists(_lib.lib_path()) else _lib.lib()
    assert hasattr(L, 'n2nmn_features_expand') and hasattr(L, 'n2nmn_features_narrow')


def shared_imdb(root, n=37):
    """the 37-question CLEVR imdb of data_reader_cases with questions 3j, 3j+1, 3j+2 asking about one image"""
    imdb, params = DC.build(root, 'clevr', n=n)
    for i, info in enumerate(imdb):
        info['feature_path'] = imdb[3 * (i // 3)]['feature_path']
    params = dict(params, assembler=DC.TokenTable(
        ['_Scene', '_Find', '_Filter', '_FindSameProperty', '_Transform', '_And', '_Or', '_Count', '_Exist',
         '_EqualNum', '_MoreNum', '_LessNum', '_SameProperty', '_Describe', '<eos>']))
    return imdb, params


def batches_of(imdb, params, **extra):
    r = DataReader(None, imdb=imdb, shuffle=False, one_pass=True, **dict(params, **extra))
    out = list(r.batches())
    r.close()
    return out


@pytest.fixture()
def count_loads(monkeypatch):
    calls = []
    real = np.load

    def counting(path, *a, **k):
        calls.append(str(path))
        return real(path, *a, **k)
    monkeypatch.setattr(data_reader.np, 'load', counting)
    return calls


def test_dedupe_reader_delivers_one_row_per_image(tmp_path, count_loads):
    imdb, params = shared_imdb(str(tmp_path))
    plain = batches_of(imdb, params)
    assert [b['seq_length_batch'].shape[0] for b in plain] == [5] * 7 + [2]
    loader = data_reader.BatchLoaderClevr(imdb, dict(params, dedupe_features=True))
    bs = params['batch_size']
    for i, want in enumerate(plain):
        ids = np.arange(i * bs, min((i + 1) * bs, len(imdb)))
        del count_loads[:]
        b = loader.load_one_batch(ids)
        paths = []
        for sid in ids:
            if imdb[sid]['feature_path'] not in paths:
                paths.append(imdb[sid]['feature_path'])
        assert count_loads == paths                      # once per distinct path, in order of first occurrence
        feat, index = b['image_feat_batch'], b['image_index_batch']
        assert feat.dtype == np.float32 and feat.shape == (len(paths),) + want['image_feat_batch'].shape[1:]
        assert index.dtype == np.int32 and index.shape == (len(ids),)
        assert [paths[j] for j in index] == [imdb[sid]['feature_path'] for sid in ids]
        assert np.array_equal(feat[index].view(np.uint32), want['image_feat_batch'].view(np.uint32))
        for j, p in enumerate(paths):
            assert np.array_equal(feat[j:j + 1], np.load(p))
        for key in ('input_seq_batch', 'seq_length_batch', 'gt_layout_batch', 'answer_label_batch'):
            assert np.array_equal(b[key], want[key])
    # ... and through the prefetch thread: the same batches
    for got, want in zip(batches_of(imdb, params, dedupe_features=True), plain):
        assert np.array_equal(got['image_feat_batch'][got['image_index_batch']], want['image_feat_batch'])
    assert len(plain[-1]['seq_length_batch']) == 2


def test_plain_reader_is_unchanged(tmp_path, count_loads):
    imdb, params = shared_imdb(str(tmp_path))
    del count_loads[:]
    loader = data_reader.BatchLoaderClevr(imdb, params)
    assert len(count_loads) == 1                         # (the constructor reads the grid's shape)
    b = loader.load_one_batch(np.arange(5))
    assert len(count_loads) == 1 + 5                     # once per question, as the reference does
    assert 'image_index_batch' not in b
    assert sorted(b) == ['answer_label_batch', 'gt_layout_batch', 'image_feat_batch', 'image_path_list',
                         'input_seq_batch', 'seq_length_batch']
    assert b['image_feat_batch'].dtype == np.float32 and b['image_feat_batch'].shape == (5, 3, 4, 8)
    for n in range(5):
        assert np.array_equal(b['image_feat_batch'][n:n + 1], np.load(imdb[n]['feature_path']))
    for opts in (dict(feature_dtype=None, dedupe_features=False), dict(feature_dtype='float32')):
        c = data_reader.BatchLoaderClevr(imdb, dict(params, **opts)).load_one_batch(np.arange(5))
        assert sorted(c) == sorted(b) and c['image_feat_batch'].dtype == np.float32
        assert np.array_equal(c['image_feat_batch'], b['image_feat_batch'])
    with pytest.raises(ValueError, match='float16'):
        data_reader.BatchLoaderClevr(imdb, dict(params, feature_dtype='bfloat16'))


def test_half_reader_rounds_fp32_files_and_keeps_fp16_files(tmp_path):
    imdb, params = DC.build(str(tmp_path), 'clevr', n=7)
    params = dict(params, load_gt_layout=False)
    files = [np.load(info['feature_path']) for info in imdb]
    # file 2 is stored as half already, with bit patterns a float32 round trip would still keep -- and one it
    # need not: a signalling NaN (0x7d01) comes through only if the loader does not touch the values
    h = files[2].astype(np.float16)
    h.reshape(-1).view(np.uint16)[:4] = (0x0001, 0x8000, 0x7c00, 0x7d01)
    np.save(imdb[2]['feature_path'], h)
    # file 3: fp32 values that sit exactly between two halves (ties go to the even neighbour), the largest
    # value that still rounds to 65504, a tie at the bottom of the subnormals
    f = files[3].copy()
    f.reshape(-1)[:4] = (1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.996, 2.0 ** -25)
    np.save(imdb[3]['feature_path'], f)
    b = data_reader.BatchLoaderClevr(imdb, dict(params, feature_dtype='float16')).load_one_batch(np.arange(7))
    feat = b['image_feat_batch']
    assert feat.dtype == np.float16 and feat.shape == (7, 3, 4, 8) and 'image_index_batch' not in b
    for n in range(7):
        want = h if n == 2 else (f if n == 3 else files[n]).astype(np.float16)
        assert np.array_equal(feat[n:n + 1].view(np.uint16), want.view(np.uint16)), n
    got = feat[3].reshape(-1)[:4]
    assert got[0] == 1.0 and got[1] == np.float16(1.0 + 2.0 ** -9) and got[2] == 65504 and got[3] == 0
    # both options together, into caller-owned staging arrays of the reader's dtype
    for info in imdb[4:]:
        info['feature_path'] = imdb[4]['feature_path']
    loader = data_reader.BatchLoaderClevr(imdb, dict(params, feature_dtype='float16', dedupe_features=True))
    out = dict(image_feat_batch=np.full((7, 3, 4, 8), 9, np.float16), image_index_batch=np.full((7,), -1, np.int32))
    b = loader.load_one_batch(np.arange(7), out=out)
    assert b['image_feat_batch'].base is out['image_feat_batch'] and b['image_feat_batch'].shape[0] == 5
    assert list(b['image_index_batch']) == [0, 1, 2, 3, 4, 4, 4] and b['image_index_batch'].base is out['image_index_batch']
    assert np.array_equal(b['image_feat_batch'][b['image_index_batch']].view(np.uint16)[:5], feat[:5].view(np.uint16))
    assert (out['image_feat_batch'][5:] == 9).all()      # rows behind U are not the batch's


def test_engine_features_checks_a_host_index_before_any_device_call():
    """Engine.features on an object that has NO device, context or library: the checks of a host index come
    first, so they raise before anything could touch the GPU"""
    from n2nmn_amd.engine import Engine
    eng = object.__new__(Engine)
    feat = np.zeros((3, 2, 2, 8), np.float16)
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
        Engine.features(eng, feat, np.array([0, 1, 3], np.int32))
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
        Engine.features(eng, feat.astype(np.float32), [0, -1, 2])
    with pytest.raises(ValueError, match='4 entries'):
        Engine.features(eng, feat, np.array([0, 1, 2], np.int32), n=4)
    with pytest.raises(ValueError, match='1-D'):
        Engine.features(eng, feat, np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match='integers'):
        Engine.features(eng, feat, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match='need an image index'):
        Engine.features(eng, feat, None, n=4)
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):     # the same check in front of a batch
        Engine._batch_features(eng, dict(image_feat_batch=feat, image_index_batch=np.array([0, 5], np.int32),
                                         seq_length_batch=np.ones(2, np.int32)))
    # a valid index gets past the checks and only then needs the device this object does not have
    with pytest.raises(AttributeError):
        Engine.features(eng, feat, np.array([2, 0, 0, 1], np.int32))
