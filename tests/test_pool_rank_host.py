"""Full-pool ranks, host side (no GPU): the restatement of nnr_pool_ranks (tests/pool_rank_ref.py) against a literal double loop, the
metrics against their formulas, the refusals of ops.pool_ranks that come before any launch, the entry point's own argument refusals with
the workspace size, and rank_in_pool's refusals by message."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pool_rank_ref as P
import recommend_ref as R


def _ints(rng, n, D):
    return rng.integers(-2, 3, size=(n, D)).astype(np.float32)


@pytest.mark.parametrize('n_user,n_reps,D', [(1, 1, 1), (3, 7, 2), (4, 9, 3), (2, 5, 3), (5, 20, 1)])
def test_restatement_against_the_double_loop(n_user, n_reps, D):
    """Integer entries in -2..2: float64 sums are exact and ties are everywhere.  Every user gets a different number of targets (the first
    none), one target twice; with a pool mask, with exclusion lists that hold pads, duplicates and entries outside the table, and both."""
    rng = np.random.default_rng(100 * n_user + n_reps)
    user, reps = _ints(rng, n_user, D), _ints(rng, n_reps, D)
    valid = (rng.random(n_reps) < 0.7).astype(np.uint8)
    ex = rng.integers(-2, n_reps + 2, size=(n_user, 4)).astype(np.int32)
    ex[:, 1] = ex[:, 0]
    ex[0, 2] = -1
    counts = np.arange(n_user) * 2 if n_user > 1 else np.array([3])
    t_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    t_news = rng.integers(0, n_reps, size=int(t_off[-1])).astype(np.int32)
    t_news[-1] = t_news[-2]                                                      # one target twice
    for v, e in ((None, None), (valid, None), (None, ex), (valid, ex)):
        el = R.eligible(n_user, n_reps, v, e)
        ahead, pool = P.ranks(R.scores64(user, reps), el, t_off, t_news)
        e_naive = None if e is None else [[r for r in row if 0 <= r < n_reps] for row in e.tolist()]
        nah, npool = P.ranks_naive(user.tolist(), reps.tolist(), t_off, t_news, v, e_naive)
        np.testing.assert_array_equal(ahead, nah)
        np.testing.assert_array_equal(pool, npool)
        assert ahead[-1] == ahead[-2] and ((ahead == -1) == ~el[P._user_of(t_off), t_news]).all()
        # the place in recommend_ref's unbounded list is the same number
        idx, _ = R.topk(R.scores64(user, reps), el, n_reps)
        for j, (u, t) in enumerate(zip(P._user_of(t_off), t_news)):
            where = np.nonzero(idx[u] == t)[0]
            assert (ahead[j] == -1 and where.size == 0) or (where.size == 1 and where[0] == ahead[j])
        lo, hi = P.bracket(user, reps, el, t_off, t_news)                        # the exact answer lies inside its own bracket
        assert ((lo <= ahead) & (ahead <= hi))[ahead >= 0].all() and (lo[ahead < 0] == -1).all()


def test_restatement_on_equal_scores_and_an_empty_pool():
    user, reps = np.ones((2, 3), dtype=np.float32), np.ones((6, 3), dtype=np.float32)
    t_off, t_news = [0, 3, 6], [0, 5, 2, 4, 4, 1]
    ahead, pool = P.ranks(R.scores64(user, reps), R.eligible(2, 6), t_off, t_news)
    np.testing.assert_array_equal(ahead, [0, 5, 2, 4, 4, 1])                    # all scores equal: the rows before it
    np.testing.assert_array_equal(pool, [6, 6])
    valid = np.array([0, 1, 0, 0, 1, 1], dtype=np.uint8)
    ahead, pool = P.ranks(R.scores64(user, reps), R.eligible(2, 6, valid, np.array([[4], [-1]])), t_off, t_news)
    np.testing.assert_array_equal(ahead, [-1, 1, -1, 1, 1, 0])
    np.testing.assert_array_equal(pool, [2, 3])
    ahead, pool = P.ranks(R.scores64(user, reps), R.eligible(2, 6, np.zeros(6, dtype=np.uint8)), t_off, t_news)
    assert (ahead == -1).all() and (pool == 0).all()


def test_metrics_match_their_formulas():
    """Hand-made vectors; evaluate.pool_rank_metrics (device-agnostic torch, float64) gives the restatement's numbers."""
    from nnr_amd import evaluate as E
    ahead = np.array([0, 4, 5, 9, 10, -1, 2, -1, 0], dtype=np.int32)
    pool = np.array([100, 100, 6, 10, 11, 50, 1, 0, 1], dtype=np.int32)
    m = P.metrics(ahead, pool)
    assert m['counted'] == 7 and m['skipped'] == 2
    assert m['hr@5'] == 4 / 7 and m['hr@10'] == 6 / 7
    assert m['ndcg@5'] == pytest.approx((1 + 1 / math.log2(6) + 1 / math.log2(4) + 1) / 7, rel=1e-15)
    assert m['ndcg@10'] == pytest.approx((1 + 1 / math.log2(6) + 1 / math.log2(7) + 1 / math.log2(11) + 1 / math.log2(4) + 1) / 7, rel=1e-15)
    assert m['mrr'] == pytest.approx((1 + 1 / 5 + 1 / 6 + 1 / 10 + 1 / 11 + 1 / 3 + 1) / 7, rel=1e-15)
    # pool_size > 1: the first five counted targets (the two with pool_size 1 are left out of the percentile only)
    assert m['percentile'] == pytest.approx((1 + (1 - 4 / 99) + (1 - 5 / 5) + (1 - 9 / 9) + (1 - 10 / 10)) / 5, rel=1e-15)
    for ks in ((5, 10), (1, 3, 64)):
        want = P.metrics(ahead, pool, ks)
        got = E.pool_rank_metrics(torch.from_numpy(ahead), torch.from_numpy(pool), ks)
        assert set(got) == set(want) and got['counted'] == want['counted'] and got['skipped'] == want['skipped']
        assert all(isinstance(v, float) for k, v in got.items() if k not in ('counted', 'skipped'))
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-14), k
    best = P.metrics([0, 0], [7, 2])
    assert all(best[k] == 1.0 for k in ('hr@5', 'ndcg@5', 'hr@10', 'ndcg@10', 'mrr', 'percentile'))
    for m in (P.metrics([-1, -1, -1], [5, 0, 9]), E.pool_rank_metrics(torch.tensor([-1, -1, -1]), torch.tensor([5, 0, 9]))):
        assert m['counted'] == 0 and m['skipped'] == 3                          # everything skipped: NaN, not an error
        assert all(math.isnan(m[k]) for k in ('hr@5', 'ndcg@5', 'hr@10', 'ndcg@10', 'mrr', 'percentile'))


def test_wrapper_refusals_come_before_any_launch():
    """CPU tensors throughout: a call that got as far as the library would be refused for them (the last cases), so every earlier message
    shows that its check ran first."""
    from nnr_amd import ops, _lib
    u, r = torch.zeros(3, 8), torch.zeros(5, 8)
    i32 = torch.int32
    off = lambda *v: torch.tensor(v, dtype=i32)
    cases = [
        (dict(user=u.double()), 'float32 tables'), (dict(reps=torch.zeros(5, 7)), 'float32 tables'),
        (dict(user=torch.zeros(8, 3).t()), 'not adjacent'), (dict(reps=torch.zeros(0, 8)), 'empty input'),
        (dict(valid=torch.ones(4, dtype=torch.uint8)), 'valid must be'), (dict(exclude=torch.zeros(3, 2, dtype=torch.int64)), 'exclude must be'),
        (dict(exclude=torch.zeros(1, 2, dtype=i32).expand(3, 2)), 'rows overlap'), (dict(user=torch.zeros(1, 8).expand(3, 8)), 'overlapping rows'),
        (dict(t_off=off(0, 1, 1, 2).long()), 'contiguous int32'), (dict(t_news=torch.tensor([0, 4])), 'contiguous int32'),
        (dict(t_news=torch.tensor([0, 9, 4, 9], dtype=i32)[::2]), 'contiguous int32'), (dict(t_off=off(0, 1, 1, 2).view(2, 2)), 'contiguous int32'),
        (dict(t_off=off(0, 1, 2)), 't_off has 3 entries for 3 user rows'), (dict(t_off=off(0, 0, 1, 1, 2)), 't_off has 5 entries'),
        (dict(t_off=off(0, 2, 1, 2)), 'non-decreasing from 0'), (dict(t_off=off(1, 1, 1, 2)), 'non-decreasing from 0'),
        (dict(t_off=off(0, 1, 1, 3)), 'non-decreasing from 0'), (dict(t_off=off(0, 1, 1, 1)), 'non-decreasing from 0'),
        (dict(t_news=torch.tensor([0, 5], dtype=i32)), 't_news outside 0 .. 4'), (dict(t_news=torch.tensor([-1, 4], dtype=i32)), 't_news outside'),
        (dict(reps=torch.full((5, 8), float('nan'))), 'finite'),
        (dict(), 'device tensors'), (dict(check=False), 'device tensors'),
    ]
    for kw, msg in cases:
        args = dict(user=u, reps=r, t_off=off(0, 1, 1, 2), t_news=torch.tensor([0, 4], dtype=i32))
        args.update(kw)
        with pytest.raises(_lib.NnrHipError, match=msg):
            ops.pool_ranks(**args)


def test_entry_point_refusals_and_workspace_size():
    """nnr_pool_ranks answers NNR_ERR_ARG / NNR_ERR_UNSUPPORTED before it touches a pointer (none of these is a device pointer);
    nnr_pool_rank_workspace_bytes is 0 where one workgroup per user tile walks all news and [n_target + n_user, splits] int32 otherwise,
    with nnr_topk_scores' number of splits."""
    from nnr_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = dict(user=p, n_user=2, ldu=4, reps=p, n_reps=5, ldr=4, D=4, valid=None, exclude=None, E=0, ld_ex=0, t_off=p, t_news=p, n_target=3,
                ahead=p, t_score=p, pool_size=p, ws=None, ws_bytes=0)
    bad = [dict(user=None), dict(reps=None), dict(ahead=None), dict(t_score=None), dict(pool_size=None), dict(t_off=None), dict(t_news=None),
           dict(n_user=0), dict(n_reps=0), dict(D=0), dict(ldu=3), dict(ldr=3), dict(E=-1), dict(E=2, ld_ex=1, exclude=p), dict(E=2, ld_ex=2),
           dict(n_target=-1), dict(n_target=0, pool_size=None), dict(n_target=0, t_off=None)]
    for over in bad:
        a = dict(good)
        a.update(over)
        assert L.nnr_pool_ranks(*a.values(), None) == _lib.NNR_ERR_ARG, over
    for over in (dict(n_reps=2 ** 31), dict(n_user=2 ** 31 - 1), dict(n_target=2 ** 31)):
        a = dict(good)
        a.update(over)
        assert L.nnr_pool_ranks(*a.values(), None) == _lib.NNR_ERR_UNSUPPORTED, over
    q = L.nnr_pool_rank_workspace_bytes
    assert q(2, 5, 3) == 0 and q(100000, 255, 7) == 0 and q(64, 383, 1000) == 0          # one, two and three news tiles never split
    assert q(0, 5, 3) == 0 and q(2, 0, 3) == 0 and q(2, 5, -1) == 0 and q(2, 2 ** 31, 3) == 0 and q(3, 3000, 2 ** 31) == 0
    for n_user, n_reps, n_target, K in ((3, 3000, 7, 10), (3, 3000, 0, 1), (200, 6000, 900, 64), (64, 42000, 64, 10), (5, 70001, 11, 5)):
        splits = L.nnr_topk_workspace_bytes(n_user, n_reps, K) // (n_user * K * 8)
        assert splits >= 2 and q(n_user, n_reps, n_target) == 4 * (n_target + n_user) * splits, (n_user, n_reps, n_target)
    assert q(3, 3000, 7) == 4 * 10 * 12                                           # 24 news tiles, two per split
    assert q(50000, 42000, 400000) == 4 * 450000 * 3                              # 782 user tiles: ceil(2048 / 782) = 3 workgroups each
    need = q(3, 3000, 3)
    a = dict(good, n_user=3, n_reps=3000)                                         # a launch that splits needs its workspace
    assert L.nnr_pool_ranks(*a.values(), None) == _lib.NNR_ERR_ARG
    a.update(ws=p, ws_bytes=need - 1)
    assert L.nnr_pool_ranks(*a.values(), None) == _lib.NNR_ERR_ARG
    a.update(ws=p + 2, ws_bytes=need)
    assert L.nnr_pool_ranks(*a.values(), None) == _lib.NNR_ERR_ARG
    assert L.nnr_tape_fn_id(b'nnr_pool_ranks') >= 0 and L.nnr_tape_fn_id(b'nnr_pool_rank_workspace_bytes') < 0


def _model(news, user, extra=()):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    cfg = make_config(['--news_encoder=' + news, '--user_encoder=' + user, *extra], corpus_sizes=dict(vocabulary_size=50, user_num=5))
    return Model(cfg)


def test_rank_in_pool_refuses_by_name_before_it_reads_the_corpus():
    from nnr_amd import evaluate as E, _lib
    for news, user, extra in (('CNE', 'SUE', ()), ('CNN', 'CATT', ()), ('HDC', 'FIM', ('--click_predictor=FIM',))):
        model = _model(news, user, extra).train()
        why = E.recommend_refusal(model)
        assert why
        E.LAST_STATS.clear()
        with pytest.raises(_lib.NnrHipError) as e:
            E.rank_in_pool(model, None, [0], [1])
        assert str(e.value) == why and model.training and not E.LAST_STATS
        model.eval()
        with pytest.raises(_lib.NnrHipError):
            E.rank_in_pool(model, None, [0], [1])
        assert not model.training
