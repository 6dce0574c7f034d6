"""Listwise evaluation, the parts that need no GPU (nnr_amd.evaluate.list_plan / listwise_supported, the encoders' candidate_independent flag,
the float64 restatement of nnr_list_scores and the entry point's refusals)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import list_eval_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [[3, 4, 6, 4, 3], [1], [8], [9], [1, 17, 2]]          # the first: the sizes of tests/golden/eval_tiny_*.npz


def test_restatement_equals_the_naive_double_loop():
    for D, n, nu, nr in ((1, 1, 3, 3), (5, 7, 3, 4), (65, 9, 3, 3)):
        ub, rb, row, cand = list_eval_ref.tables(nu, nr, D, n, D + 3, D + 2, seed=D)
        got = list_eval_ref.list_scores(ub[:, :D], rb[:, :D], row, cand)
        exp = list_eval_ref.list_scores_naive(ub[:, :D], rb[:, :D], row, cand)
        assert got.dtype == np.float64 and np.isfinite(got).all()
        np.testing.assert_allclose(got, exp, rtol=0, atol=1e-13 * max(1.0, float(np.abs(exp).max())))    # (another order of 65 float64 terms)
        assert list_eval_ref.list_scores(ub[:, :D], rb[:, :D], row, cand, np.float32).dtype == np.float32


@pytest.mark.parametrize('sizes', SIZES)
@pytest.mark.parametrize('K', [1, 3, 8])
def test_list_plan_candidate_aware(sizes, K):
    from nnr_amd.evaluate import list_plan
    p = list_plan(sizes, K)
    n, n_imp = sum(sizes), len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    imp = np.repeat(np.arange(n_imp), sizes)
    np.testing.assert_array_equal(p.first, first)
    np.testing.assert_array_equal(p.imp, imp)
    R = p.row_imp.shape[0]
    assert p.row_slots.shape == p.slot_valid.shape == (R, K) and p.row.dtype == np.int32 and p.row.shape == (n,)
    # the rows of impression i number ceil(size_i / K), in impression order
    np.testing.assert_array_equal(np.bincount(p.row_imp, minlength=n_imp), [-(-s // K) for s in sizes])
    assert (np.diff(p.row_imp) >= 0).all()
    # every sample sits in exactly one non-pad slot
    flat, valid = p.row_slots.reshape(-1), p.slot_valid.reshape(-1)
    np.testing.assert_array_equal(np.sort(flat[valid]), np.arange(n))
    # every slot, pad slots included, names a sample of the row's own impression; a pad slot holds the row's first sample
    np.testing.assert_array_equal(imp[p.row_slots], np.broadcast_to(p.row_imp[:, None], (R, K)))
    assert p.slot_valid[:, 0].all()
    np.testing.assert_array_equal(p.row_slots[~p.slot_valid], np.broadcast_to(p.row_slots[:, :1], (R, K))[~p.slot_valid])
    # row, restricted to the non-pad slots, is a bijection: slot row[j] holds j, and the slots hit are exactly the non-pad ones
    np.testing.assert_array_equal(flat[p.row], np.arange(n))
    np.testing.assert_array_equal(np.sort(p.row), np.flatnonzero(valid))


@pytest.mark.parametrize('sizes', SIZES)
def test_list_plan_independent(sizes):
    """K = None: one user row per impression, no slots -- a row serves every sample of its impression."""
    from nnr_amd.evaluate import list_plan
    p = list_plan(sizes, None)
    imp = np.repeat(np.arange(len(sizes)), sizes)
    np.testing.assert_array_equal(p.row, imp)
    np.testing.assert_array_equal(p.imp, imp)
    np.testing.assert_array_equal(p.first, np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    np.testing.assert_array_equal(p.row_imp, np.arange(len(sizes)))
    assert p.row.dtype == np.int32 and p.row_slots is None and p.slot_valid is None and p.candidates_per_row is None


def test_list_plan_refuses_empty_impressions():
    from nnr_amd.evaluate import list_plan
    for bad in ([], [3, 0, 2], [-1]):
        with pytest.raises(ValueError):
            list_plan(bad, 8)
    with pytest.raises(ValueError):
        list_plan([3], 0)


def test_candidate_independent_flag_table():
    from nnr_amd import user_encoders as U
    classes = {n: c for n, c in inspect.getmembers(U, inspect.isclass) if issubclass(c, U.UserEncoder) and c is not U.UserEncoder}
    assert set(classes) == {'SUE', 'SUE_wo_GCN', 'SUE_wo_HCA', 'MHSA', 'ATT', 'GRU', 'CATT', 'OMAP', 'PUE', 'FIM'}
    assert U.UserEncoder.candidate_independent is False
    assert {n for n, c in classes.items() if c.candidate_independent} == {'ATT', 'MHSA', 'GRU', 'PUE', 'SUE_wo_HCA'}


@pytest.mark.parametrize('news,user,ok', [('CNE', 'SUE', False), ('CNE_wo_CA', 'ATT', False), ('PNE', 'PUE', False),
                                          ('CNN', 'ATT', True), ('MHSA', 'SUE', True), ('CNE_wo_CS', 'ATT', True)])
def test_listwise_supported(news, user, ok):
    from nnr_amd import evaluate as E
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    m = Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user], corpus_sizes=dict(vocabulary_size=50, user_num=7)))
    assert E.listwise_supported(m) is ok and E.news_reps_cacheable(m) is ok
    if not ok:                                                   # refused before the corpus is looked at, naming the reason
        with pytest.raises(Exception, match='batch_independent') as e:
            E.compute_scores_listwise(m, None, [1], 8)
        assert news in str(e.value)


def test_entry_point_is_declared_listed_recordable_and_refuses_bad_arguments():
    from nnr_amd import _lib, evaluate, ops
    header = open(os.path.join(ROOT, 'include', 'nnr_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert re.search(r'\bnnr_list_scores\s*\(', header) and 'l ^ 32' in header
    assert 'nnr_list_scores' in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), 'nnr_list_scores')
    L = _lib.lib()
    assert L.nnr_tape_fn_id(b'nnr_list_scores') >= 0
    assert callable(ops.list_scores) and callable(evaluate.compute_scores_listwise)
    # the refusals need no device: nothing is launched, no pointer is read (the non-null ones below point at host memory)
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    good = dict(user=p, n_user=3, ldu=4, reps=p, n_reps=3, ldr=4, row=p, cand=p, n=5, D=4, scores=p)
    order = ('user', 'n_user', 'ldu', 'reps', 'n_reps', 'ldr', 'row', 'cand', 'n', 'D', 'scores')
    bad = [dict(user=None), dict(reps=None), dict(row=None), dict(cand=None), dict(scores=None), dict(n=0), dict(n=-3), dict(D=0), dict(D=-1),
           dict(ldu=3), dict(ldr=3), dict(n_user=0), dict(n_reps=0), dict(n_user=-1), dict(n_reps=-1),
           dict(user=None, reps=None, row=None, cand=None, scores=None, n=0, D=0)]
    for over in bad:
        a = dict(good, **over)
        assert L.nnr_list_scores(*[a[k] for k in order], None) == _lib.NNR_ERR_ARG, over
    assert (buf == 0).all()
