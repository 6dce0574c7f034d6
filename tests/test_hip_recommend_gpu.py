"""Top-K recommendation on the device (nnr_amd.ops.topk_scores / csrc/topk.hip, nnr_amd.evaluate.recommend) against the float64
restatement of tests/recommend_ref.py.

Bars.  Integer inputs in -2..2 make every partial sum exact in fp32 in any order: idx and score must EQUAL the restatement, ties and cut
included.  Random inputs are judged by float64 through recommend_ref.band_check with b(u, r) = D * 2^-23 * sum_d |u_d r_d|, the bound of
an fp32 fused-multiply-add sum of D terms in any order with a factor 2 of slack; nothing is left out of that check.  Position independence
is to the bit.  Every measured figure is printed.

The kernel tiles 64 users x 128 news, streams D in slabs of 32, and gives every news split at least two tiles: the shapes below cross
each of those edges (1, 31, 33, 65 users; 1, 31, 129, 1031, 3000 news; D = 1, 3, 30, 37, 64, 100, 500), run one workgroup over several tiles
(129 news), several splits with a merge (1031, 3000), and both load paths (16-byte: aligned tables whose D and strides are multiples of
4; 4-byte: everything else)."""
import functools

import numpy as np
import pytest
import torch

import recommend_ref as R

pytestmark = pytest.mark.gpu


def _place(a, pad, off):
    """`a` [n, D] on the device as a view with row stride D + pad whose first element sits `off` floats behind an aligned allocation; the
    gaps hold NaN (a kernel that read them would show it)."""
    n, D = a.shape
    flat = torch.full((n * (D + pad) + off,), float('nan'), device='cuda')
    view = flat[off:].view(n, D + pad)[:, :D]
    view.copy_(torch.from_numpy(np.array(a)))                                   # (a copy: the shared inputs are read-only)
    return view


def _run(user, reps, K, valid=None, exclude=None, pad=3, off=1, rpad=None):
    """ops.topk_scores on a user table of row stride D + pad and a news table of row stride D + rpad (default pad + 2), both `off` floats
    behind an aligned allocation."""
    from nnr_amd import ops
    v = None if valid is None else torch.from_numpy(np.asarray(valid, dtype=np.uint8)).cuda()
    e = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).cuda()
    idx, score = ops.topk_scores(_place(user, pad, off), _place(reps, pad + 2 if rpad is None else rpad, off), K, valid=v, exclude=e)
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == tuple(score.shape) == (user.shape[0], K)
    return idx.cpu().numpy(), score.cpu().numpy()


def _ints(seed, n, D):
    return np.random.default_rng(seed).integers(-2, 3, size=(n, D)).astype(np.float32)


def _exact(user, reps, K, valid=None, exclude=None, **kw):
    el = R.eligible(len(user), len(reps), valid, exclude)
    eidx, esc = R.topk(R.scores64(user, reps), el, K)
    idx, sc = _run(user, reps, K, valid, exclude, **kw)
    np.testing.assert_array_equal(idx, eidx)
    np.testing.assert_array_equal(sc, esc.astype(np.float32))
    return idx, sc


# ------------------------------------------------------------------------------------------------------------------ 1. exact arithmetic
@pytest.mark.parametrize('n_reps', [1, 31, 129, 1031])
@pytest.mark.parametrize('D', [1, 3, 30, 64])
def test_integer_inputs_give_the_exact_answer(D, n_reps):
    """Row strides D + 3 and D + 5 with both tables one float off their allocations (4-byte loads), and at D = 64 also strides 68 and 72 on
    aligned tables (16-byte loads with strides larger than D).  Scores are small integers, so almost every comparison inside the kernel is a
    tie."""
    for n_user in (1, 33, 65):
        user, reps = _ints(1000 * D + n_user, n_user, D), _ints(7 * D + n_reps, n_reps, D)
        for K in (1, 5, 64):
            for pad, off, rpad in ((3, 1, 5),) + (((4, 0, 8),) if D % 4 == 0 else ()):
                assert (pad == 3) or ((D + pad) % 4 == 0 and (D + rpad) % 4 == 0)       # the second layout is the 16-byte path's
                _exact(user, reps, K, pad=pad, off=off, rpad=rpad)


def test_long_news_ranges_walk_many_tiles_per_split():
    """70 001 news are 547 tiles for at most 256 splits: every workgroup walks two or three tiles and the merge folds 256 lists."""
    user, reps = _ints(5, 5, 3), _ints(6, 70001, 3)
    assert np.abs(user[0]).sum() > 0
    reps[69990:, :] = 3.0 * np.sign(user[0])                                    # user 0's best rows stand at the very end (3 > every other entry)
    idx, _ = _exact(user, reps, 5)
    np.testing.assert_array_equal(idx[0], np.arange(69990, 69995))


# ------------------------------------------------------------------------------------------------------------------ 2. random inputs
@functools.lru_cache(maxsize=None)
def _normal(D):
    """(user [70, D], reps [3000, D], float64 scores, bound): drawn once per D, then only read."""
    rng = np.random.default_rng(40 + D)
    user, reps = rng.standard_normal((70, D)).astype(np.float32), rng.standard_normal((3000, D)).astype(np.float32)
    for a in (user, reps):
        a.setflags(write=False)
    return user, reps, R.scores64(user, reps), R.bound(user, reps)


@pytest.mark.parametrize('D', [100, 500])
def test_normal_inputs_against_float64(D):
    user, reps, _, _ = _normal(D)
    el = R.eligible(70, 3000)
    for pad, off in ((0, 0), (3, 1)):
        idx, sc = _run(user, reps, 10, pad=pad, off=off)
        a, c = R.band_check(user, reps, el, 10, idx, sc)
        print('D %d pad %d off %d: worst |score - float64| / b = %.3f, worst omitted excess / band = %.3f' % (D, pad, off, a, c))


@pytest.mark.parametrize('D', [1, 37, 100, 500])
def test_a_score_is_the_fmaf_chain_of_the_header(D):
    """include/nnr_hip.h states the summation order: acc = fmaf(user[u, d], reps[r, d], acc) over d ascending from +0.  recommend_ref.fma_chain32
    is that chain on the host, every step rounded once (tests/test_recommend_host.py checks it against exact rational arithmetic); with
    K = 64 = n_reps the kernel returns every pair's score, which must have the chain's bits -- on the 4-byte path (stride D + 3, off by one
    float), on the 16-byte path where D allows it, and with the news beyond the first tile (rows 130.. of a table whose other rows are out
    of the pool)."""
    rng = np.random.default_rng(70 + D)
    user, reps = rng.standard_normal((5, D)).astype(np.float32), rng.standard_normal((64, D)).astype(np.float32)
    chain = R.fma_chain32(user, reps)
    assert chain.dtype == np.float32 and (D == 1 or (chain != (user.astype(np.float64) @ reps.astype(np.float64).T).astype(np.float32)).any())
    layouts = [dict(pad=3, off=1)] + ([dict(pad=4, off=0, rpad=8), dict(pad=0, off=0, rpad=0)] if D % 4 == 0 else [])
    for kw in layouts:
        idx, sc = _run(user, reps, 64, **kw)
        got = np.empty_like(sc)
        np.put_along_axis(got, idx.astype(np.int64), sc, axis=1)
        assert (np.sort(idx, axis=1) == np.arange(64)).all()
        bad = int((got.view(np.uint32) != chain.view(np.uint32)).sum())
        print('D %d %r: %d of %d scores differ from the host chain' % (D, kw, bad, got.size))
        assert bad == 0, (D, kw, bad)
    big = rng.standard_normal((64 + 190, D)).astype(np.float32)
    big[130:194] = reps
    valid = np.zeros(len(big), dtype=np.uint8)
    valid[130:194] = 1
    idx, sc = _run(user, big, 64, valid=valid)
    got = np.empty_like(sc)
    np.put_along_axis(got, idx.astype(np.int64) - 130, sc, axis=1)
    assert (got.view(np.uint32) == chain.view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------------------------ 3. position independence
def _pairs(idx, sc):
    return {(u, int(r)): sc[u, k].view(np.uint32) for u in range(idx.shape[0]) for k, r in enumerate(idx[u]) if r >= 0}


def _same_where_both_and_sets_agree_outside_the_band(D, name, a, b):
    """a, b: (idx, score) of two launches over the same (user, news) pairs, rows already mapped to _normal(D)'s numbering."""
    _, _, s64, bnd = _normal(D)
    pa, pb = _pairs(*a), _pairs(*b)
    both = set(pa) & set(pb)
    assert len(both) >= 0.9 * len(pa)
    differ = [p for p in both if pa[p] != pb[p]]
    assert not differ, '%s: %d of %d scores differ in their bits, e.g. %r' % (name, len(differ), len(both), differ[:3])
    for (x, y) in ((a, b), (b, a)):
        for u in range(x[0].shape[0]):
            last = int(y[0][u, -1])
            for r in set(x[0][u].tolist()) - set(y[0][u].tolist()):               # in one list only: a tie of float64 inside the band
                assert abs(s64[u, r] - s64[u, last]) <= bnd[u, r] + bnd[u, last], (name, u, r)
    print('%s: %d pairs in both lists, bit-identical' % (name, len(both)))


@pytest.mark.parametrize('D', [100, 500])
def test_a_score_is_a_pure_function_of_its_two_rows(D):
    """Users 0..2 of the 70 (so that the launch splits the news over workgroups): alone; at rows 5..7 of a user table of 11 and with the
    news at rows 77.. of a table of 3150 whose other rows are out of the pool (other tiles, other splits, the other load path); and with
    the news table reversed.  The first three rows of the 70-user launch are a fourth statement of the same pairs."""
    user, reps, _, _ = _normal(D)
    rng = np.random.default_rng(9)
    base = _run(user[:3], reps, 10, pad=0, off=0)
    full = _run(user, reps, 10, pad=0, off=0)
    _same_where_both_and_sets_agree_outside_the_band(D, 'D %d: 3 users / 70 users' % D, base, (full[0][:3], full[1][:3]))
    big_u, big_r = rng.standard_normal((11, D)).astype(np.float32), rng.standard_normal((3150, D)).astype(np.float32)
    big_u[5:8], big_r[77:3077] = user[:3], reps
    valid = np.zeros(3150, dtype=np.uint8)
    valid[77:3077] = 1
    idx, sc = _run(big_u, big_r, 10, valid=valid)
    assert ((idx[5:8] >= 77) & (idx[5:8] < 3077)).all()
    _same_where_both_and_sets_agree_outside_the_band(D, 'D %d: embedded at other offsets' % D, base, (idx[5:8] - 77, sc[5:8]))
    idx, sc = _run(user[:3], np.ascontiguousarray(reps[::-1]), 10, pad=0, off=0)
    _same_where_both_and_sets_agree_outside_the_band(D, 'D %d: news table reversed' % D, base, (2999 - idx, sc))


# ------------------------------------------------------------------------------------------------------------------ 4. eligibility
@pytest.mark.parametrize('n_reps', [300, 1031])
def test_eligibility(n_reps):
    """300 news: one workgroup walks three tiles; 1031: four splits and the merge.  33 users, D = 3, integer inputs, K = 5 and 64."""
    n_user = 33
    user, reps = _ints(21, n_user, 3), _ints(22 + n_reps, n_reps, 3)
    stride = (np.arange(n_reps) % 3 == 1).astype(np.uint8)
    edges = [0, 31, 32, 127, 128, n_reps - 1]
    rng = np.random.default_rng(23)
    ex = rng.integers(0, n_reps, size=(n_user, 14)).astype(np.int32)
    ex[:, :6] = edges                                                           # entries on tile boundaries, for every user
    ex[:, 6] = ex[:, 7]                                                         # a duplicate
    ex[:, 8], ex[:, 9], ex[:, 10] = -1, n_reps, n_reps + 5                      # a pad and entries outside the table
    ex[::2, 11] = -7
    for K in (5, 64):
        _exact(user, reps, K, valid=stride)
        idx, sc = _exact(user, reps, K, valid=np.zeros(n_reps, dtype=np.uint8))
        assert (idx == -1).all() and np.isneginf(sc).all()
        idx, _ = _exact(user, reps, K, exclude=ex)
        assert not np.isin(idx, edges).any()
        _exact(user, reps, K, valid=stride, exclude=ex)
        top, _ = R.topk(R.scores64(user, reps), R.eligible(n_user, n_reps), K)   # the would-be top K, all excluded
        idx, _ = _exact(user, reps, K, exclude=top)
        assert all(not set(idx[u].tolist()) & set(top[u].tolist()) for u in range(n_user))
    few = np.zeros(n_reps, dtype=np.uint8)
    few[[31, 128, n_reps - 1]] = 1                                              # three rows in the pool, one of them excluded for user 0
    one = np.full((n_user, 1), -1, dtype=np.int32)
    one[0, 0] = 128
    idx, sc = _exact(user, reps, 5, valid=few, exclude=one)
    assert (idx[1:, 3:] == -1).all() and (idx[1:, :3] >= 0).all() and (idx[0, 2:] == -1).all() and np.isneginf(sc[:, 3:]).all()


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def _split():
    """A synthetic corpus of 300 news with short titles and 40 behaviours over 25 distinct (user, history) rows."""
    from nnr_amd.corpus import from_synth_lists
    from nnr_amd.synth import SynthSpec, SynthCorpus
    spec = SynthSpec(vocabulary_size=500, news_pool=300, max_title_length=12, max_abstract_length=24, max_history_num=10,
                     title_len_mean=6.0, content_len_mean=10.0, seed=8)
    rng = np.random.default_rng(12)
    return from_synth_lists(SynthCorpus(spec), np.ones(40, dtype=np.int64), rng, 'cuda', distinct_users=25), spec


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


@pytest.mark.parametrize('news,user', [('CNN', 'ATT'), ('MHSA', 'MHSA'), ('CNN', 'PUE')])
def test_recommend_end_to_end(news, user):
    from nnr_amd import evaluate as E, ops
    dc, _ = _split()
    model = _e2e_model(news, user)
    t = dc.t
    hist, hmask = t['beh_history'].cpu().numpy().astype(np.int64), t['beh_history_mask'].cpu().numpy() != 0
    n = hist.shape[0]
    pool = np.unique(np.concatenate([np.random.default_rng(2).choice(np.arange(1, 300), size=50, replace=False), hist[hmask][:10]]))
    assert pool.size <= 64 and np.isin(hist[hmask], pool).any()
    res = {}
    for ex in (True, False):
        for dd in (True, False):
            news_i, sc = E.recommend(model, dc, 64, pool=pool, exclude_history=ex, dedup_users=dd)
            st = dict(E.LAST_STATS)
            assert model.training and news_i.dtype == torch.int64 and sc.dtype == torch.float32 and tuple(news_i.shape) == tuple(sc.shape) == (n, 64)
            assert st['mode'] == 'recommend' and st['rows'] == n and st['pool'] == pool.size and st['K'] == 64 and st['encoder_rows'] >= pool.size
            assert st['user_rows'] == n if not dd else 1 <= st['user_rows'] <= 25
            res[ex, dd] = news_i.cpu().numpy(), sc.cpu().numpy()
        assert res[ex, True][0].tobytes() == res[ex, False][0].tobytes() and res[ex, True][1].tobytes() == res[ex, False][1].tobytes()
    # the judge: this package's own user and news tables through nnr_list_scores' inputs, in float64
    model.eval()
    with torch.no_grad():
        ids = torch.from_numpy(pool).cuda()
        reps = E.encode_news_table(model, dc, ids)
        used, inv = torch.unique(t['beh_history'].long().reshape(-1), return_inverse=True)
        table = E._user_table(model, dc, E.encode_news_table(model, dc, used), t['beh_user'], t['beh_history'].long(), t['beh_history_mask'] != 0,
                              inv.view_as(t['beh_history']), None, 16)
        row = torch.arange(n, device='cuda', dtype=torch.int32).repeat_interleave(pool.size)
        cand = torch.arange(pool.size, device='cuda', dtype=torch.int32).repeat(n)
        listed = ops.list_scores(table, reps, row, cand).view(n, pool.size).cpu().numpy()
    model.train()
    U, Rp = table.cpu().numpy(), reps.cpu().numpy()
    s64, b = R.scores64(U, Rp), R.bound(U, Rp)
    assert (np.abs(listed - s64) <= b).all()
    col = {int(v): j for j, v in enumerate(pool)}
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
            assert (np.abs(sc[u, :len(j)].astype(np.float64) - s64[u, j]) <= b[u, j]).all(), (u, 'score band')
            assert (np.abs(sc[u, :len(j)].astype(np.float64) - listed[u, j]) <= b[u, j]).all(), (u, 'against nnr_list_scores')
            k = sc[u, :len(j)]
            assert ((k[:-1] > k[1:]) | ((k[:-1] == k[1:]) & (got[:-1] < got[1:]))).all(), (u, 'ranked by its own scores, ties by news index')
            d64 = s64[u, j]
            wrong = (d64[:-1] < d64[1:]) & (d64[1:] - d64[:-1] > b[u, j[:-1]] + b[u, j[1:]])
            assert not wrong.any(), (u, 'order outside the band')
        assert seen_history == (not ex)
    print('%s+%s: %d rows, pool %d' % (news, user, n, pool.size))


def test_the_user_row_reaches_a_personalised_encoder():
    """Two behaviour rows with one history and two users: PUE (the user embedding is the attention query) must rank for each of them on its
    own, ATT (which never reads the user) must give both the same bits.  De-duplication keeps them apart either way: the user is part of the
    row's key."""
    import copy
    from nnr_amd import evaluate as E
    dc, _ = _split()
    two = copy.copy(dc)
    two.t = dict(dc.t)
    counts = (dc.t['beh_history_mask'] != 0).sum(dim=1)
    src = int(torch.argmax(counts))                                             # the fullest history
    for k in ('beh_user', 'beh_history', 'beh_history_mask'):
        two.t[k] = dc.t[k].clone()
    for k in ('beh_history', 'beh_history_mask'):
        two.t[k][0], two.t[k][1] = dc.t[k][src], dc.t[k][src]
    two.t['beh_user'][0], two.t['beh_user'][1] = 3, 17
    assert int(counts[src]) >= 3 and torch.equal(two.t['beh_history'][0], two.t['beh_history'][1])
    for user, differ in (('PUE', True), ('ATT', False)):
        model = _e2e_model('CNN', user)
        if differ:
            assert not torch.equal(model.user_embedding.weight[3], model.user_embedding.weight[17])
        news_i, sc = E.recommend(model, two, 20, rows=[0, 1])
        assert E.LAST_STATS['user_rows'] == 2
        same = torch.equal(sc[0], sc[1]) and torch.equal(news_i[0], news_i[1])
        print('CNN+%s: rows of one history and two users give %s' % (user, 'the same bits' if same else 'different scores'))
        assert same != differ, user


def test_recommend_rows_and_default_pool():
    """rows picks behaviour rows (repeats allowed, any order); the default pool is every news but PAD news 0."""
    from nnr_amd import evaluate as E
    dc, _ = _split()
    model = _e2e_model('CNN', 'ATT')
    all_n, all_s = E.recommend(model, dc, 7)
    assert E.LAST_STATS['pool'] == 299 and int(all_n.min()) >= 1 and tuple(all_n.shape) == (40, 7)
    rows = [5, 0, 5, 39]
    n2, s2 = E.recommend(model, dc, 7, rows=rows)
    assert torch.equal(n2, all_n[rows]) and torch.equal(s2, all_s[rows]) and E.LAST_STATS['rows'] == 4
    with pytest.raises(ValueError, match='rows'):
        E.recommend(model, dc, 7, rows=[40])
    with pytest.raises(ValueError, match='pool'):
        E.recommend(model, dc, 7, pool=[300])


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_on_the_device():
    from nnr_amd import evaluate as E, ops, _lib
    dc, _ = _split()
    for news, user, word in (('CNE', 'SUE', 'batch_independent'), ('CNN', 'CATT', 'candidate_independent')):
        model = _e2e_model(news, user)
        E.LAST_STATS.clear()
        with pytest.raises(_lib.NnrHipError, match=word):
            E.recommend(model, dc, 5)
        assert not E.LAST_STATS and model.training
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    fim = Model(make_config(['--news_encoder=HDC', '--user_encoder=FIM', '--click_predictor=FIM'], corpus_sizes=dict(vocabulary_size=500))).cuda()
    with pytest.raises(_lib.NnrHipError, match='dot_product'):
        E.recommend(fim, dc, 5)
    u, r = torch.randn(3, 8, device='cuda'), torch.randn(40, 8, device='cuda')
    with pytest.raises(_lib.NnrHipError, match='unsupported'):
        ops.topk_scores(u, r, 65)
    with pytest.raises(_lib.NnrHipError, match='finite'):
        ops.topk_scores(u, torch.full((40, 8), float('inf'), device='cuda'), 5)
    idx, sc = ops.topk_scores(u, r, 64)
    assert int((idx >= 0).sum()) == 3 * 40 and bool(torch.isneginf(sc[:, 40:]).all())
