"""The archive form of top-K recommendation and full-pool ranks on the device (nnr_topk_archive_scores / nnr_pool_archive_ranks through
nnr_amd.ops.topk_scores / pool_ranks with archives=, csrc/topk.hip; evaluate.recommend / rank_in_pool for OMAP) against the float64
restatement of tests/archive_rank_ref.py.

Bars.  One archive: the bits of the plain entry points.  Integer inputs with scale = 0 and 2 or 4 archives: means of small integers are
exact, so idx and score EQUAL the restatement, ties, cut, short pools and tails included.  Equal archives: the bits of the plain launch on
the single row.  Normal inputs: archive_rank_ref.band_check with the band B of that module, nothing left out; every worst ratio is printed.
A combined score is a pure function of its A + 1 rows and the scale, to the bit: positions, strides, load path, splits, and whether the
tile walk or the rank pre-pass computed it.

The kernel tiles 64 users x 128 news, streams D in slabs of 32 once per archive, and gives every news split at least two tiles: 1, 3, 5,
65, 70 users; 1, 31, 129, 1031 news (one tile, several tiles in one workgroup, four splits and the merge); D = 1, 3, 30, 64, 100, 500; the
16-byte path (aligned tables whose D, lda and strides are multiples of 4) and the 4-byte path (everything else)."""
import copy
import functools

import numpy as np
import pytest
import torch

import archive_rank_ref as AR
import pool_rank_ref as P
import recommend_ref as R

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _place(a, pad, off):
    """`a` [n, D] as a device view of row stride D + pad, `off` floats behind an aligned allocation; the gaps hold NaN."""
    n, D = a.shape
    flat = torch.full((n * (D + pad) + off,), NAN, device='cuda')
    view = flat[off:].view(n, D + pad)[:, :D]
    view.copy_(torch.from_numpy(np.array(a)))
    return view


def _place3(a, lpad=0, upad=0, off=0):
    """`a` [n, A, D] as a device view with lda = D + lpad and ldu = A * lda + upad, `off` floats behind an aligned allocation; gaps NaN."""
    n, A, D = a.shape
    lda = D + lpad
    ldu = A * lda + upad
    flat = torch.full((n * ldu + off,), NAN, device='cuda')
    view = flat.as_strided((n, A, D), (ldu, lda, 1), off)
    view.copy_(torch.from_numpy(np.array(a)))
    return view


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _topk(user3, reps, K, scale, valid=None, exclude=None, lpad=0, upad=0, off=0, rpad=0):
    from nnr_amd import ops
    idx, sc = ops.topk_scores(_place3(user3, lpad, upad, off), _place(reps, rpad, off), K, valid=_dev(valid, np.uint8),
                              exclude=_dev(exclude, np.int32), archives=user3.shape[1], scale=scale)
    assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and tuple(idx.shape) == tuple(sc.shape) == (user3.shape[0], K)
    return idx.cpu().numpy(), sc.cpu().numpy()


def _ranks(user3, reps, t_off, t_news, scale, valid=None, exclude=None, lpad=0, upad=0, off=0, rpad=0):
    from nnr_amd import ops
    a, s, p = ops.pool_ranks(_place3(user3, lpad, upad, off), _place(reps, rpad, off), _dev(t_off, np.int32), _dev(t_news, np.int32),
                             valid=_dev(valid, np.uint8), exclude=_dev(exclude, np.int32), archives=user3.shape[1], scale=scale)
    assert a.dtype == torch.int32 and s.dtype == torch.float32 and p.dtype == torch.int32 and tuple(p.shape) == (user3.shape[0],)
    return a.cpu().numpy(), s.cpu().numpy(), p.cpu().numpy()


LAYOUTS = (dict(lpad=0, upad=0, off=0, rpad=0), dict(lpad=3, upad=2, off=1, rpad=5), dict(lpad=4, upad=8, off=0, rpad=8))


def _layouts(D):
    """Packed (16-byte loads when D % 4 == 0), odd strides one float off (4-byte loads), and padded strides on the 16-byte path."""
    return LAYOUTS if D % 4 == 0 else LAYOUTS[:2]


def _ints(seed, *shape):
    return np.random.default_rng(seed).integers(-2, 3, size=shape).astype(np.float32)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ 1. one archive
@pytest.mark.parametrize('D', [3, 64, 100])
@pytest.mark.parametrize('n_reps', [129, 1031])
def test_one_archive_has_the_bits_of_the_plain_entry_points(n_reps, D):
    from nnr_amd import ops
    for n_user in (3, 70):
        rng = np.random.default_rng(D * 7 + n_reps + n_user)
        user, reps = rng.standard_normal((n_user, 1, D)).astype(np.float32), rng.standard_normal((n_reps, D)).astype(np.float32)
        valid = (np.arange(n_reps) % 5 != 2).astype(np.uint8)
        ex = rng.integers(-1, n_reps + 2, size=(n_user, 6)).astype(np.int32)
        t_off = (np.arange(n_user + 1) * 9).astype(np.int32)
        t_news = rng.integers(0, n_reps, size=n_user * 9).astype(np.int32)
        ex[:, 0] = t_news[::9]                                                  # every user's first target is in its own exclusion list
        for lay in _layouts(D):
            u2, r = _place(user[:, 0], lay['lpad'] + lay['upad'], lay['off']), _place(reps, lay['rpad'], lay['off'])
            v, e, to, tn = _dev(valid, np.uint8), _dev(ex, np.int32), _dev(t_off, np.int32), _dev(t_news, np.int32)
            pidx, psc = ops.topk_scores(u2, r, 10, valid=v, exclude=e)
            pa, ps, pp = ops.pool_ranks(u2, r, to, tn, valid=v, exclude=e)
            aidx, asc = _topk(user, reps, 10, 0.37, valid, ex, **lay)
            aa, as_, ap = _ranks(user, reps, t_off, t_news, 0.37, valid, ex, **lay)
            np.testing.assert_array_equal(aidx, pidx.cpu().numpy())
            np.testing.assert_array_equal(_bits(asc), _bits(psc.cpu().numpy()))
            np.testing.assert_array_equal(aa, pa.cpu().numpy())
            np.testing.assert_array_equal(_bits(as_), _bits(ps.cpu().numpy()))
            np.testing.assert_array_equal(ap, pp.cpu().numpy())
            assert (aa[::9] == -1).all() and (aa >= 0).any()


# ------------------------------------------------------------------------------------------------------------------ 2. exact arithmetic
@pytest.mark.parametrize('n_reps', [1, 31, 129, 1031])
@pytest.mark.parametrize('D', [1, 3, 30, 64])
def test_integer_inputs_with_scale_zero_give_the_exact_answer(D, n_reps):
    """Scores are means of 2 or 4 small integers: exact, and almost every comparison inside the kernel is a tie.  Bare, and with a pool
    mask and exclusion lists (pads, rows outside the table, duplicates)."""
    for A in (2, 4):
        for n_user in (1, 65):
            user, reps = _ints(1000 * D + 10 * n_user + A, n_user, A, D), _ints(7 * D + n_reps, n_reps, D)
            rng = np.random.default_rng(D + n_reps + A)
            valid = (np.arange(n_reps) % 3 != 1).astype(np.uint8)
            ex = rng.integers(-1, n_reps + 2, size=(n_user, 5)).astype(np.int32)
            ex[:, 4] = ex[:, 3]
            s64 = AR.scores64(user, reps, 0.0)
            for v, e in ((None, None), (valid, ex)):
                el = AR.eligible(n_user, n_reps, v, e)
                for K in (1, 10, 64):
                    want_i, want_s = AR.topk(s64, el, K)
                    for lay in _layouts(D)[:2] if K != 10 else _layouts(D):
                        idx, sc = _topk(user, reps, K, 0.0, v, e, **lay)
                        np.testing.assert_array_equal(idx, want_i)
                        np.testing.assert_array_equal(sc, want_s.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ 3. equal archives
@pytest.mark.parametrize('A', [2, 4])
def test_equal_archives_have_the_bits_of_the_single_row(A):
    from nnr_amd import ops
    for D, scale in ((100, 0.1), (37, -0.8)):
        rng = np.random.default_rng(A + D)
        one, reps = rng.standard_normal((70, 1, D)).astype(np.float32), rng.standard_normal((1031, D)).astype(np.float32)
        user = np.repeat(one, A, axis=1)
        pidx, psc = ops.topk_scores(_place(one[:, 0], 0, 0), _place(reps, 0, 0), 64)
        t_news = pidx.reshape(-1).contiguous()
        t_off = torch.arange(71, device='cuda', dtype=torch.int32) * 64
        for lay in _layouts(D):
            idx, sc = _topk(user, reps, 64, scale, **lay)
            np.testing.assert_array_equal(idx, pidx.cpu().numpy())
            np.testing.assert_array_equal(_bits(sc), _bits(psc.cpu().numpy()))
            ahead, ts, _ = ops.pool_ranks(_place3(user, lay['lpad'], lay['upad'], lay['off']), _place(reps, lay['rpad'], lay['off']), t_off, t_news,
                                          archives=A, scale=scale)
            assert torch.equal(ts.view(torch.int32), psc.reshape(-1).view(torch.int32))
            assert torch.equal(ahead.view(70, 64), torch.arange(64, device='cuda', dtype=torch.int32).expand(70, 64))


# ------------------------------------------------------------------------------------------------------------------ 4. normal inputs
@functools.lru_cache(maxsize=None)
def _normal(A, D):
    """(user [70, A, D], reps [1031, D], scale, float64 scores, band): drawn once per (A, D), then only read."""
    rng = np.random.default_rng(40 + 17 * A + D)
    user, reps = rng.standard_normal((70, A, D)).astype(np.float32), rng.standard_normal((1031, D)).astype(np.float32)
    for a in (user, reps):
        a.setflags(write=False)
    scale = float(1.0 / np.sqrt(D))
    return user, reps, scale, AR.scores64(user, reps, scale), AR.band(user, reps, scale)


@pytest.mark.parametrize('D', [100, 500])
@pytest.mark.parametrize('A', [2, 3, 16])
def test_normal_inputs_against_float64(A, D):
    user, reps, scale, s64, band = _normal(A, D)
    valid = (np.arange(1031) % 11 != 4).astype(np.uint8)
    for K, v, lay in ((10, None, LAYOUTS[0]), (64, valid, LAYOUTS[1])):
        idx, sc = _topk(user, reps, K, scale, v, **lay)
        a, c = AR.band_check(s64, band, AR.eligible(70, 1031, v), K, idx, sc)
        print('A %d D %d K %d %r: worst |score - float64| / B = %.4f, worst omitted excess / band = %.3f' % (A, D, K, lay, a, c))


# ------------------------------------------------------------------------------------------------------------------ 5. pure function
@pytest.mark.parametrize('A,D', [(3, 100), (16, 36), (2, 101)])
def test_a_score_is_a_pure_function_of_its_rows_and_the_scale(A, D):
    """Five users and 64 news, every pair's score returned (K = 64 = the pool, the other rows of the news table masked out), in four
    settings: alone, with the news scattered over a table of 1031 rows (four splits and the merge); at rows 31..35 of a table of 70 users
    (two user tiles) with the news at other rows, hence in other tiles and splits; alone, with padded strides on the 16-byte path (where D
    allows it); among the 70 again, one float off an aligned allocation with odd strides (4-byte loads).  And in every setting once more
    from the rank pre-pass: t_score of every pair."""
    rng = np.random.default_rng(A * D)
    user, news = rng.standard_normal((5, A, D)).astype(np.float32), rng.standard_normal((64, D)).astype(np.float32)
    scale = 1.7 / np.sqrt(D)
    seen = []
    for k, (n_user, first, lay) in enumerate(((5, 0, LAYOUTS[0]), (70, 31, LAYOUTS[0]), (5, 0, LAYOUTS[2]), (70, 31, LAYOUTS[1]))):
        if lay is LAYOUTS[2] and D % 4:
            continue
        where = np.sort(rng.choice(1031, size=64, replace=False))
        big_u, big_r = rng.standard_normal((n_user, A, D)).astype(np.float32), rng.standard_normal((1031, D)).astype(np.float32)
        big_u[first:first + 5], big_r[where] = user, news
        valid = np.zeros(1031, dtype=np.uint8)
        valid[where] = 1
        idx, sc = _topk(big_u, big_r, 64, scale, valid, **lay)
        idx, sc = idx[first:first + 5], sc[first:first + 5]
        assert (np.sort(idx, axis=1) == where).all()
        got = np.empty((5, 64), dtype=np.float32)
        np.put_along_axis(got, np.searchsorted(where, idx), sc, axis=1)        # by news, not by rank
        seen.append(('top-K, setting %d' % k, got))
        t_off = np.zeros(n_user + 1, dtype=np.int32)
        t_off[first + 1:first + 6] = 64 * np.arange(1, 6)
        t_off[first + 6:] = 320
        ahead, ts, pool = _ranks(big_u, big_r, t_off, np.tile(where, 5), scale, valid, **lay)
        assert (pool == 64).all() and (np.sort(ahead.reshape(5, 64), axis=1) == np.arange(64)).all()
        seen.append(('pre-pass, setting %d' % k, ts.reshape(5, 64)))
    err = np.abs(seen[0][1].astype(np.float64) - AR.scores64(user, news, scale)) / AR.band(user, news, scale)
    assert err.max() <= 1.0
    for name, got in seen[1:]:
        bad = int((_bits(got) != _bits(seen[0][1])).sum())
        print('A %d D %d %s: %d of 320 scores differ from setting 0' % (A, D, name, bad))
        assert bad == 0, name


# ------------------------------------------------------------------------------------------------------------------ 6. ranks
@pytest.mark.parametrize('A,D', [(3, 100), (16, 500)])
def test_ranks_agree_with_the_top_k_list_and_the_float64_bracket(A, D):
    user, reps, scale, s64, band = _normal(A, D)
    rng = np.random.default_rng(A + D)
    for lay in (LAYOUTS[0], LAYOUTS[1]):
        idx, sc = _topk(user, reps, 64, scale, **lay)
        t_off = np.arange(71, dtype=np.int32) * 64
        ahead, ts, pool = _ranks(user, reps, t_off, idx.reshape(-1), scale, **lay)
        np.testing.assert_array_equal(ahead.reshape(70, 64), np.tile(np.arange(64, dtype=np.int32), (70, 1)))
        np.testing.assert_array_equal(_bits(ts.reshape(70, 64)), _bits(sc))
        assert (pool == 1031).all()
        rand = rng.integers(0, 1031, size=(70, 20)).astype(np.int32)
        t_off = np.arange(71, dtype=np.int32) * 20
        ahead, ts, _ = _ranks(user, reps, t_off, rand.reshape(-1), scale, **lay)
        ahead = ahead.reshape(70, 20)
        listed = np.array([[t in set(idx[u].tolist()) for t in rand[u]] for u in range(70)])
        assert ((ahead < 64) == listed).all() and (ahead >= 0).all()
        hit = np.nonzero(listed)
        assert (idx[hit[0], ahead[hit]] == rand[hit]).all() and (_bits(sc[hit[0], ahead[hit]]) == _bits(ts.reshape(70, 20)[hit])).all()
        lo, hi = AR.bracket(s64, band, AR.eligible(70, 1031), t_off, rand.reshape(-1))
        assert ((lo <= ahead.reshape(-1)) & (ahead.reshape(-1) <= hi)).all()
        print('A %d D %d %r: %d of %d random targets inside the top 64; widest bracket %d' % (A, D, lay, int(listed.sum()), listed.size,
                                                                                            int((hi - lo).max())))


@pytest.mark.parametrize('A', [2, 4])
def test_more_targets_than_the_lds_block_holds_and_users_without_targets(A):
    """70 users x 1031 news (two user tiles, four splits): the even users of the first tile have 80 targets each (2560 > 2048, so the
    counters beyond the block live in the workspace), the odd ones none; the second tile's users have three.  Every user's first target is
    in its own exclusion list.  Integer inputs and scale = 0: the counts equal the restatement."""
    rng = np.random.default_rng(A)
    user, reps = _ints(3 + A, 70, A, 3), _ints(4, 1031, 3)
    per = [80 if u < 64 and u % 2 == 0 else (0 if u < 64 else 3) for u in range(70)]
    t_off = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    t_news = rng.integers(0, 1031, size=int(t_off[-1])).astype(np.int32)
    ex = np.full((70, 2), -1, dtype=np.int32)
    for u in range(70):
        if per[u]:
            ex[u, 1] = t_news[t_off[u]]
    valid = (np.arange(1031) % 5 != 2).astype(np.uint8)
    el = AR.eligible(70, 1031, valid, ex)
    s64 = AR.scores64(user, reps, 0.0)
    want, wpool = AR.ranks(s64, el, t_off, t_news)
    assert sum(per[:64]) > 2048 and (want[t_off[:-1][np.array(per) > 0]] == -1).all()
    for lay in (LAYOUTS[1], dict(lpad=1, upad=0, off=0, rpad=1)):
        ahead, ts, pool = _ranks(user, reps, t_off, t_news, 0.0, valid, ex, **lay)
        np.testing.assert_array_equal(ahead, want)
        np.testing.assert_array_equal(pool, wpool)
        np.testing.assert_array_equal(ts, s64[P._user_of(t_off), t_news].astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_on_the_device():
    from nnr_amd import _lib, ops
    reps = torch.randn(40, 8, device='cuda')
    t_off, t_news = torch.tensor([0, 1, 1, 2], device='cuda', dtype=torch.int32), torch.tensor([3, 4], device='cuda', dtype=torch.int32)
    for user, kw, word in ((torch.randn(3, 8, device='cuda'), dict(archives=0), 'archives'),
                           (torch.randn(3, 17 * 8, device='cuda'), dict(archives=17), 'unsupported'),
                           (torch.randn(3, 24, device='cuda'), dict(archives=3, lda=7), 'lda'),
                           (torch.randn(3, 23, device='cuda'), dict(archives=3), 'archives'),
                           (torch.randn(3, 2, 8, device='cuda')[:, :1].expand(3, 3, 8), dict(archives=3), 'overlapping'),
                           (torch.full((3, 24), float('inf'), device='cuda'), dict(archives=3), 'finite'),
                           (torch.randn(3, 24, device='cuda'), dict(archives=3, scale=float('inf')), 'scale')):
        with pytest.raises(_lib.NnrHipError, match=word):
            ops.topk_scores(user, reps, 5, **kw)
        with pytest.raises(_lib.NnrHipError, match=word):
            ops.pool_ranks(user, reps, t_off, t_news, **kw)
    user = torch.randn(3, 3, 8, device='cuda')
    with pytest.raises(_lib.NnrHipError, match='unsupported'):
        ops.topk_scores(user, reps, 65, archives=3, scale=0.2)
    gaps = torch.full((3, 30), NAN, device='cuda')                              # NaN between the archives is not part of the table
    gaps.view(3, 3, 10)[:, :, :8] = user
    idx, sc = ops.topk_scores(gaps, reps, 64, archives=3, lda=10, scale=0.2)
    idx2, sc2 = ops.topk_scores(user, reps, 64, archives=3, scale=0.2)
    assert torch.equal(idx, idx2) and torch.equal(sc.view(torch.int32), sc2.view(torch.int32))
    assert int((idx >= 0).sum()) == 3 * 40 and bool(torch.isneginf(sc[:, 40:]).all())
    L = _lib.lib()                                                              # the entry points themselves, with device pointers
    out_i, out_s = torch.zeros(3 * 5, device='cuda', dtype=torch.int32), torch.zeros(3 * 5, device='cuda')
    for A, lda, ldu, scale, rc in ((0, 8, 24, 0.5, _lib.NNR_ERR_ARG), (17, 8, 17 * 8, 0.5, _lib.NNR_ERR_UNSUPPORTED), (3, 7, 24, 0.5, _lib.NNR_ERR_ARG),
                                   (3, 8, 23, 0.5, _lib.NNR_ERR_ARG), (3, 8, 24, NAN, _lib.NNR_ERR_ARG)):
        got = L.nnr_topk_archive_scores(user.data_ptr(), 3, ldu, A, lda, scale, reps.data_ptr(), 40, 8, 8, None, None, 0, 0, 5, out_i.data_ptr(),
                                        out_s.data_ptr(), None, 0, None)
        assert got == rc, (A, lda, ldu, scale, got)
    torch.cuda.synchronize()
    assert not out_i.any() and not out_s.any()


# ------------------------------------------------------------------------------------------------------------------ 8. end to end
@functools.lru_cache(maxsize=None)
def _split():
    """A synthetic corpus of 300 news and 40 behaviours over 25 distinct (user, history) rows; behaviour row 0 has no history at all and
    row 1 two live slots of ten (the generator's own rows are padded too)."""
    from nnr_amd.corpus import from_synth_lists
    from nnr_amd.synth import SynthSpec, SynthCorpus
    spec = SynthSpec(vocabulary_size=500, news_pool=300, max_title_length=12, max_abstract_length=24, max_history_num=10,
                     title_len_mean=6.0, content_len_mean=10.0, seed=8)
    dc = from_synth_lists(SynthCorpus(spec), np.ones(40, dtype=np.int64), np.random.default_rng(12), 'cuda', distinct_users=25)
    own = copy.copy(dc)
    own.t = dict(dc.t)
    for k in ('beh_history', 'beh_history_mask'):
        own.t[k] = dc.t[k].clone()
    own.t['beh_history'][0] = 0
    own.t['beh_history_mask'][0] = 0
    own.t['beh_history'][1, :2] = torch.tensor([17, 230], device='cuda', dtype=own.t['beh_history'].dtype)
    own.t['beh_history'][1, 2:] = 0
    own.t['beh_history_mask'][1] = 0
    own.t['beh_history_mask'][1, :2] = 1
    return own, spec


def _e2e_model(news, user):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    _, spec = _split()
    cfg = make_config(['--news_encoder=' + news, '--user_encoder=' + user, '--max_title_length=%d' % spec.max_title_length,
                       '--max_abstract_length=%d' % spec.max_abstract_length, '--max_history_num=%d' % spec.max_history_num],
                      corpus_sizes=dict(vocabulary_size=spec.vocabulary_size, user_num=40))
    torch.manual_seed(1)
    model = Model(cfg)
    model.initialize()
    return model.cuda().train()


@pytest.mark.parametrize('news', ['CNN', 'MHSA'])
def test_recommend_and_rank_in_pool_end_to_end_for_omap(news):
    from nnr_amd import _lib, evaluate as E, ops
    from nnr_amd.user_encoders import _omap_forward
    dc, _ = _split()
    model = _e2e_model(news, 'OMAP')
    ue = model.user_encoder
    A = ue.OMAP_head_num
    marker = object()
    ue.auxiliary_loss = marker
    t = dc.t
    hist, hmask = t['beh_history'].cpu().numpy().astype(np.int64), t['beh_history_mask'].cpu().numpy() != 0
    n = hist.shape[0]
    assert not hmask[0].any() and hmask[1].sum() == 2 and any(0 < m.sum() < 10 for m in hmask[2:])
    clicked = dc.samples[:, 0].cpu().numpy().astype(np.int64)
    pool = np.unique(np.concatenate([np.random.default_rng(2).choice(np.arange(1, 300), size=36, replace=False), hist[hmask][:10], clicked[:16]]))
    assert 40 <= pool.size <= 64 and np.isin(hist[hmask], pool).any() and not np.isin(clicked, pool).all()
    E.LAST_STATS.clear()
    for call in (lambda: E.recommend(model, dc, 64, pool=pool), lambda: E.rank_in_pool(model, dc, [0], [int(pool[0])], pool=pool)):
        with pytest.raises(_lib.NnrHipError, match='archives=True'):            # without the keyword: refused, as before the archive form
            call()
    assert not E.LAST_STATS and model.training and ue.auxiliary_loss is marker
    res = {}
    for ex in (True, False):
        for dd in (True, False):
            news_i, sc = E.recommend(model, dc, 64, pool=pool, exclude_history=ex, dedup_users=dd, archives=True)
            st = dict(E.LAST_STATS)
            assert model.training and ue.auxiliary_loss is marker
            assert news_i.dtype == torch.int64 and sc.dtype == torch.float32 and tuple(news_i.shape) == tuple(sc.shape) == (n, 64)
            assert st['mode'] == 'recommend' and st['archives'] == A and st['rows'] == n and st['pool'] == pool.size and st['K'] == 64
            assert st['user_rows'] == n if not dd else 1 <= st['user_rows'] <= 27
            res[ex, dd] = news_i.cpu().numpy(), sc.cpu().numpy()
        assert res[ex, True][0].tobytes() == res[ex, False][0].tobytes() and res[ex, True][1].tobytes() == res[ex, False][1].tobytes()
    # the judges: float64 over the archive table, and the model's OWN scoring of the same pairs (encode_user with the pool as candidates)
    model.eval()
    with torch.no_grad():
        ids = torch.from_numpy(pool).cuda()
        used, inv = torch.unique(torch.cat([t['beh_history'].long().reshape(-1), ids]), return_inverse=True)
        reps_all = E.encode_news_table(model, dc, used)
        slot_h, slot_p = inv[:n * hist.shape[1]].view(n, -1), inv[n * hist.shape[1]:]
        hm = t['beh_history_mask'] != 0
        arch = ue.encode_archives(reps_all[slot_h], hm.contiguous())
        assert tuple(arch.shape) == (n, A, reps_all.shape[1]) and ue.auxiliary_loss is marker
        own_table = E._user_table(model, dc, reps_all, t['beh_user'], t['beh_history'].long(), hm, slot_h, slot_p.view(1, -1).expand(n, -1), 16)
        reps = reps_all[slot_p].contiguous()
        row = torch.arange(n * pool.size, device='cuda', dtype=torch.int32)
        cand = torch.arange(pool.size, device='cuda', dtype=torch.int32).repeat(n)
        listed = ops.list_scores(own_table, reps, row, cand).view(n, pool.size).cpu().numpy()
        # encode_archives has the bits of the forward path's R: the user vectors of encode_user are gamma R of exactly these archives
        R_fwd = _omap_forward(ue, reps_all[slot_h], reps[None].expand(n, -1, -1), hm)[6]
        assert torch.equal(R_fwd.view(torch.int32), arch.view(torch.int32))
    model.train()
    U3, Rp = arch.cpu().numpy(), reps.cpu().numpy()
    scale = float(ue.archive_scale)
    assert abs(scale - 1.0 / np.sqrt(U3.shape[2])) < 1e-12
    s64, band = AR.scores64(U3, Rp, scale), AR.band(U3, Rp, scale)
    own3 = own_table.cpu().numpy().reshape(n, pool.size, -1).astype(np.float64)   # recommend_ref.bound of the pair (user vector for news j, news j)
    own_b = own3.shape[2] * 2.0 ** -23 * (np.abs(own3) * np.abs(Rp.astype(np.float64))[None]).sum(axis=2)
    col = {int(v): j for j, v in enumerate(pool)}
    worst = worst_own = 0.0
    for ex in (True, False):
        news_i, sc = res[ex, True]
        seen_history = False
        for u in range(n):
            live = set(hist[u][hmask[u]].tolist())
            want = [v for v in pool.tolist() if not (ex and v in live)]
            got = news_i[u][news_i[u] >= 0]
            assert sorted(got.tolist()) == sorted(want), (u, 'the whole eligible pool, once each')
            assert (news_i[u, len(want):] == -1).all() and np.isneginf(sc[u, len(want):]).all()
            seen_history |= bool(live & set(got.tolist()))
            j = np.array([col[int(v)] for v in got], dtype=np.int64)
            k = sc[u, :len(j)]
            assert ((k[:-1] > k[1:]) | ((k[:-1] == k[1:]) & (got[:-1] < got[1:]))).all(), (u, 'ranked by its own scores, ties by news index')
            e64 = np.abs(k.astype(np.float64) - s64[u, j]) / band[u, j]
            eown = np.abs(k.astype(np.float64) - listed[u, j]) / (band[u, j] + own_b[u, j])
            assert e64.max() <= 1.0, (u, 'score band', float(e64.max()))
            assert eown.max() <= 1.0, (u, 'against the model\'s own scores', float(eown.max()))
            worst, worst_own = max(worst, float(e64.max())), max(worst_own, float(eown.max()))
        assert seen_history == (not ex)
    print('%s+OMAP: %d rows, pool %d, A %d: worst |score - float64| / B = %.4f, worst |score - own score| / (B + b) = %.4f'
          % (news, n, pool.size, A, worst, worst_own))
    # rank_in_pool on the clicked targets: the position in recommend's list
    rows, targets = E.clicked_targets(dc, np.ones(dc.num, dtype=np.int64))
    for ex in (True, False):
        for dd in (True, False):
            ahead, psz, metrics = E.rank_in_pool(model, dc, rows, targets, pool=pool, exclude_history=ex, dedup_users=dd, archives=True)
            assert model.training and ue.auxiliary_loss is marker and E.LAST_STATS['archives'] == A and E.LAST_STATS['mode'] == 'rank_in_pool'
            ahead, psz = ahead.cpu().numpy(), psz.cpu().numpy()
            news_i = res[ex, True][0]
            counted = 0
            for i, (r, tg) in enumerate(zip(rows.tolist(), targets.tolist())):
                pos = np.nonzero(news_i[r] == tg)[0]
                assert psz[i] == int((news_i[r] >= 0).sum())
                assert ahead[i] == (int(pos[0]) if pos.size else -1), (i, r, tg)
                counted += int(pos.size)
            assert metrics['counted'] == counted > 0
