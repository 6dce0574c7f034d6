"""Top-K recommendation, host side (no GPU): the float64 restatement of nnr_topk_scores (tests/recommend_ref.py) against a brute-force
loop, the refusals of ops.topk_scores that come before any launch, the entry point's own argument refusals, and recommend's three
refusals by message."""
import ctypes

import numpy as np
import pytest
import torch

import recommend_ref as R


def _ints(rng, n, D):
    return rng.integers(-2, 3, size=(n, D)).astype(np.float32)


@pytest.mark.parametrize('n_user,n_reps,D,K', [(1, 1, 1, 1), (3, 7, 2, 3), (4, 9, 3, 9), (2, 5, 3, 8), (5, 20, 1, 4)])
def test_restatement_against_brute_force(n_user, n_reps, D, K):
    """Integer entries in -2..2: float64 sums are exact, ties are everywhere, and the two statements must agree to the bit -- with a pool
    mask, with exclusion lists that hold pads, duplicates and entries outside the table, and with both."""
    rng = np.random.default_rng(100 * n_user + n_reps)
    user, reps = _ints(rng, n_user, D), _ints(rng, n_reps, D)
    valid = (rng.random(n_reps) < 0.7).astype(np.uint8)
    ex = rng.integers(-2, n_reps + 2, size=(n_user, 4)).astype(np.int32)
    ex[:, 1] = ex[:, 0]                                                          # a duplicate in every list
    ex[0, 2] = -1
    for v, e in ((None, None), (valid, None), (None, ex), (valid, ex)):
        el = R.eligible(n_user, n_reps, v, e)
        idx, sc = R.topk(R.scores64(user, reps), el, K)
        e_naive = None if e is None else [[r for r in row if 0 <= r < n_reps] for row in e.tolist()]
        nidx, nsc = R.topk_naive(user.tolist(), reps.tolist(), K, v, e_naive)
        np.testing.assert_array_equal(idx, nidx)
        np.testing.assert_array_equal(sc, nsc)
        assert ((idx >= 0).sum(axis=1) == np.minimum(K, el.sum(axis=1))).all()
        R.band_check(user, reps, el, K, idx, sc.astype(np.float32))              # the exact answer passes the band check


def test_restatement_on_equal_scores_short_and_empty_pools():
    user, reps = np.ones((2, 3), dtype=np.float32), np.ones((6, 3), dtype=np.float32)
    idx, sc = R.topk(R.scores64(user, reps), R.eligible(2, 6), 4)
    np.testing.assert_array_equal(idx, [[0, 1, 2, 3]] * 2)                       # all scores equal: ascending row, also at the cut
    assert (sc == 3.0).all()
    valid = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint8)
    idx, sc = R.topk(R.scores64(user, reps), R.eligible(2, 6, valid, np.array([[4], [-1]])), 3)
    np.testing.assert_array_equal(idx, [[1, -1, -1], [1, 4, -1]])                # a pool smaller than K
    assert np.isneginf(sc[idx < 0]).all() and (sc[idx >= 0] == 3.0).all()
    idx, sc = R.topk(R.scores64(user, reps), R.eligible(2, 6, np.zeros(6, dtype=np.uint8)), 2)
    assert (idx == -1).all() and np.isneginf(sc).all()                           # an empty pool
    nidx, nsc = R.topk_naive(user.tolist(), reps.tolist(), 2, np.zeros(6, dtype=np.uint8))
    assert (nidx == -1).all() and np.isneginf(nsc).all()


def test_band_check_catches_what_it_is_for():
    rng = np.random.default_rng(3)
    user, reps = rng.standard_normal((4, 50)).astype(np.float32), rng.standard_normal((40, 50)).astype(np.float32)
    el = R.eligible(4, 40, None, np.array([[0], [1], [2], [-1]]))
    idx, sc = R.topk(R.scores64(user, reps), el, 5)
    good = sc.astype(np.float32)
    a, c = R.band_check(user, reps, el, 5, idx, good)
    assert a < 0.1 and c <= 0.0                                                  # the float64 answer rounded once sits deep inside the band
    for spoil in ('score', 'order', 'omitted', 'ineligible', 'tail'):
        i2, s2 = idx.copy(), good.copy()
        if spoil == 'score':
            s2[1, 2] *= np.float32(1.01)
        elif spoil == 'order':
            i2[0, [1, 2]], s2[0, [1, 2]] = i2[0, [2, 1]], s2[0, [2, 1]]
        elif spoil == 'omitted':                                                 # the best row replaced by the first row left out
            rest = [r for r in np.argsort(-R.scores64(user, reps)[2]) if el[2, r] and r not in idx[2]]
            i2[2, :-1], s2[2, :-1] = idx[2, 1:], good[2, 1:]
            i2[2, -1], s2[2, -1] = rest[0], np.float32(R.scores64(user, reps)[2, rest[0]])
        elif spoil == 'ineligible':
            i2[0, -1], s2[0, -1] = 0, np.float32(R.scores64(user, reps)[0, 0])
        else:
            i2[3, -1], s2[3, -1] = -1, -np.inf
        with pytest.raises(AssertionError):
            R.band_check(user, reps, el, 5, i2, s2)


def _round32(x):
    """The float32 nearest to the Fraction x, ties to even, by exact comparisons."""
    from fractions import Fraction
    c = np.float32(float(x))                                                     # within an ulp or so: walk to the nearest from here
    while True:
        lo, hi = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
        best = min((lo, c, hi), key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
        if best == c:
            return c
        c = best


def test_host_fma_chain_is_correctly_rounded():
    """recommend_ref.fma32 against exact rational arithmetic rounded once: random operands, sums that cancel, and sums made to fall exactly
    on and just beside the midpoint of two float32 neighbours (where rounding the float64 sum a second time would go wrong)."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-3, 4, size=400)).astype(np.float32)
    c[:50] = (-(a[:50].astype(np.float64) * b[:50])).astype(np.float32)          # cancellation
    one, ulp = np.float32(1.0), np.float32(2.0 ** -23)
    a = np.concatenate([a, np.array([ulp / 2, ulp / 2, 2.0 ** -24 + 2.0 ** -48, 2.0 ** -24 - 2.0 ** -48, 3 * 2.0 ** -24], dtype=np.float32)])
    b = np.concatenate([b, np.array([1, 1 + ulp, 1, 1, 1], dtype=np.float32)])   # 1 + half an ulp: exactly, just above, (rounded operands), 1.5 ulp
    c = np.concatenate([c, np.full(5, one)])
    got = R.fma32(a, b, c)
    assert got.dtype == np.float32
    for i in range(a.size):
        want = _round32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i].view(np.uint32) == np.float32(want).view(np.uint32), (i, a[i], b[i], c[i], got[i], want)
    assert got[-5] == one and got[-4] == one + ulp                               # the tie goes to even, anything above it goes up
    user, reps = rng.standard_normal((2, 9)).astype(np.float32), rng.standard_normal((3, 9)).astype(np.float32)
    chain = R.fma_chain32(user, reps)
    for u in range(2):
        for r in range(3):
            acc = np.float32(0.0)
            for d in range(9):
                acc = _round32(Fraction(float(user[u, d])) * Fraction(float(reps[r, d])) + Fraction(float(acc)))
            assert chain[u, r].view(np.uint32) == np.float32(acc).view(np.uint32)


def test_wrapper_refusals_come_before_any_launch():
    """CPU tensors throughout: a call that got as far as the library would be refused for them (the last case), so every earlier message
    shows that its check ran first."""
    from nnr_amd import ops, _lib
    u, r = torch.zeros(3, 8), torch.zeros(5, 8)
    i32 = torch.int32
    cases = [
        (dict(user=u.double()), 'float32 tables'), (dict(reps=torch.zeros(5, 7)), 'float32 tables'), (dict(user=torch.zeros(8)), 'float32 tables'),
        (dict(user=torch.zeros(8, 3).t()), 'not adjacent'), (dict(reps=torch.zeros(0, 8)), 'empty input'),
        (dict(K=0), 'K = 0'), (dict(K=2.0), 'K = 2.0'),
        (dict(valid=torch.ones(4, dtype=torch.uint8)), 'valid must be'), (dict(valid=torch.ones(5)), 'valid must be'),
        (dict(valid=torch.ones(10, dtype=torch.uint8)[::2]), 'valid must be'),
        (dict(exclude=torch.zeros(3, 2, dtype=torch.int64)), 'exclude must be'), (dict(exclude=torch.zeros(2, 2, dtype=i32)), 'exclude must be'),
        (dict(exclude=torch.zeros(2, 3, dtype=i32).t()), 'exclude must be'), (dict(exclude=torch.zeros(1, 2, dtype=i32).expand(3, 2)), 'rows overlap'),
        (dict(user=torch.zeros(1, 8).expand(3, 8)), 'overlapping rows'),
        (dict(), 'device tensors'),
    ]
    for kw, msg in cases:
        args = dict(user=u, reps=r, K=2)
        args.update(kw)
        with pytest.raises(_lib.NnrHipError, match=msg):
            ops.topk_scores(**args)


def test_entry_point_refusals_and_workspace_size():
    """nnr_topk_scores answers NNR_ERR_ARG / NNR_ERR_UNSUPPORTED before it touches a pointer (none of these is a device pointer);
    nnr_topk_workspace_bytes is 0 where one workgroup per user tile walks all news and [n_user, splits, K] pairs of 4-byte words otherwise."""
    from nnr_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = dict(user=p, n_user=2, ldu=4, reps=p, n_reps=5, ldr=4, D=4, valid=None, exclude=None, E=0, ld_ex=0, K=3, idx=p, score=p, ws=None,
                ws_bytes=0)
    bad = [dict(user=None), dict(reps=None), dict(idx=None), dict(score=None), dict(n_user=0), dict(n_reps=0), dict(D=0), dict(ldu=3),
           dict(ldr=3), dict(E=-1), dict(E=2, ld_ex=1, exclude=p), dict(E=2, ld_ex=2), dict(K=0)]
    for over in bad:
        a = dict(good)
        a.update(over)
        assert L.nnr_topk_scores(*a.values(), None) == _lib.NNR_ERR_ARG, over
    a = dict(good, K=65)
    assert L.nnr_topk_scores(*a.values(), None) == _lib.NNR_ERR_UNSUPPORTED
    assert L.nnr_topk_workspace_bytes(2, 5, 3) == 0 and L.nnr_topk_workspace_bytes(100000, 255, 10) == 0
    assert L.nnr_topk_workspace_bytes(2, 5, 65) == 0 and L.nnr_topk_workspace_bytes(0, 5, 3) == 0
    need = L.nnr_topk_workspace_bytes(3, 3000, 10)
    assert need > 0 and need % (3 * 10 * 8) == 0 and 2 <= need // (3 * 10 * 8) <= 12        # 24 news tiles, at least two per split
    a = dict(good, n_user=3, n_reps=3000, K=10)                                  # a launch that splits needs its workspace
    assert L.nnr_topk_scores(*a.values(), None) == _lib.NNR_ERR_ARG
    a.update(ws=p, ws_bytes=need - 1)
    assert L.nnr_topk_scores(*a.values(), None) == _lib.NNR_ERR_ARG
    assert L.nnr_tape_fn_id(b'nnr_topk_scores') >= 0 and L.nnr_tape_fn_id(b'nnr_topk_workspace_bytes') < 0


def _model(news, user, extra=()):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    cfg = make_config(['--news_encoder=' + news, '--user_encoder=' + user, *extra], corpus_sizes=dict(vocabulary_size=50, user_num=5))
    return Model(cfg)


def test_recommend_refuses_by_name_before_it_reads_the_corpus():
    from nnr_amd import evaluate as E, _lib
    for news, user, extra, words in (('CNE', 'SUE', (), ('batch_independent', 'CNE')),
                                     ('CNN', 'CATT', (), ('candidate_independent', 'CATT', 'one encoder run per')),
                                     ('CNN', 'OMAP', (), ('candidate_independent', 'OMAP')),
                                     ('HDC', 'FIM', ('--click_predictor=FIM',), ('dot_product', 'FIM'))):
        model = _model(news, user, extra).train()
        why = E.recommend_refusal(model)
        assert why and all(w in why for w in words), (news, user, why)
        with pytest.raises(_lib.NnrHipError) as e:
            E.recommend(model, None, 5)
        assert str(e.value) == why and model.training
    assert E.recommend_refusal(_model('CNN', 'ATT')) is None and E.recommend_refusal(_model('MHSA', 'MHSA')) is None
    assert E.recommend_refusal(_model('CNN', 'PUE')) is None and 'PNE' in E.recommend_refusal(_model('PNE', 'PUE'))
