"""Full-pool ranks on the device (nnr_amd.ops.pool_ranks / csrc/topk.hip, nnr_amd.evaluate.rank_in_pool) against the restatement of
tests/pool_rank_ref.py and against this package's own top-K launch.

Bars.  Integer inputs in -2..2 make every partial sum exact in fp32 in any order: ahead, pool_size and the -1 cases must EQUAL the
restatement.  On random inputs the count is pinned three ways: to ops.topk_scores (a target's `ahead` is its position in the list and
its score has the list's bits), to itself across launch shapes (to the bit), and to float64 through pool_rank_ref.bracket, whose margin is
the two rows' recommend_ref.bound added -- derived, nothing tuned.  Every target of every case is checked.

The kernel tiles 64 users x 128 news, streams D in slabs of 32, keeps the counters of a user tile's first 2048 targets in LDS and works on
global memory beyond, and splits the news over workgroups from four news tiles on: the shapes cross each of those edges."""
import functools

import numpy as np
import pytest
import torch

import pool_rank_ref as P
import recommend_ref as R

pytestmark = pytest.mark.gpu


def _place(a, pad, off):
    """`a` [n, D] on the device as a view with row stride D + pad whose first element sits `off` floats behind an aligned allocation; the
    gaps hold NaN (a kernel that read them would show it)."""
    n, D = a.shape
    flat = torch.full((n * (D + pad) + off,), float('nan'), device='cuda')
    view = flat[off:].view(n, D + pad)[:, :D]
    view.copy_(torch.from_numpy(np.array(a)))
    return view


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _run(user, reps, t_off, t_news, valid=None, exclude=None, pad=3, off=1):
    """ops.pool_ranks on tables of row strides D + pad and D + pad + 2 (D + pad for pad = 0), `off` floats behind an aligned allocation."""
    from nnr_amd import ops
    ahead, score, pool = ops.pool_ranks(_place(user, pad, off), _place(reps, pad + 2 if pad else 0, off), _dev(t_off, np.int32),
                                        _dev(t_news, np.int32), valid=_dev(valid, np.uint8), exclude=_dev(exclude, np.int32))
    T = len(t_news)
    assert ahead.dtype == torch.int32 and score.dtype == torch.float32 and pool.dtype == torch.int32
    assert tuple(ahead.shape) == tuple(score.shape) == (T,) and tuple(pool.shape) == (user.shape[0],)
    return ahead.cpu().numpy(), score.cpu().numpy(), pool.cpu().numpy()


def _ints(seed, n, D):
    return np.random.default_rng(seed).integers(-2, 3, size=(n, D)).astype(np.float32)


def _target_lists(rng, n_user, n_reps):
    """Per user, by u % 5: no target; one; 70 (more than a wave's lanes; drawn with repeats); one target twice; the rows of the last
    (partial) news tile.  A single user gets all of them."""
    last = np.arange(128 * ((n_reps - 1) // 128), n_reps)
    kinds = [lambda: np.zeros(0, dtype=np.int64), lambda: rng.integers(0, n_reps, size=1), lambda: rng.integers(0, n_reps, size=70),
             lambda: np.repeat(rng.integers(0, n_reps, size=1), 2), lambda: last[-5:]]
    lists = [np.concatenate([k() for k in kinds])] if n_user == 1 else [kinds[u % 5]() for u in range(n_user)]
    t_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return t_off, np.concatenate(lists).astype(np.int32), lists


def _exact(user, reps, t_off, t_news, valid=None, exclude=None, **kw):
    el = R.eligible(len(user), len(reps), valid, exclude)
    want, wpool = P.ranks(R.scores64(user, reps), el, t_off, t_news)
    ahead, score, pool = _run(user, reps, t_off, t_news, valid, exclude, **kw)
    np.testing.assert_array_equal(ahead, want)
    np.testing.assert_array_equal(pool, wpool)
    tu = P._user_of(t_off)
    np.testing.assert_array_equal(score, R.scores64(user, reps)[tu, t_news].astype(np.float32))     # integers: exact in any order
    return ahead


# ------------------------------------------------------------------------------------------------------------------ 1. exact arithmetic
@pytest.mark.parametrize('D', [1, 3, 32, 33, 100])
def test_integer_inputs_give_the_exact_counts(D):
    """1, 63, 64, 65 users x 1, 127, 128, 129, 257 news.  Scores are small integers, so most comparisons are ties and the row order decides.
    Run bare, and with a pool mask (rows r % 7 == 3 out) plus exclusion lists (a user's first target, a pad, a row outside the table, three
    random rows, one of them twice): the targets that must report -1 are those the construction names, counted here by hand.  4-byte loads
    (stride D + 3, off by one float) and, where D allows, 16-byte loads."""
    total = minus = 0
    for n_user in (1, 63, 64, 65):
        for n_reps in (1, 127, 128, 129, 257):
            rng = np.random.default_rng(1000 * D + 10 * n_user + n_reps)
            user, reps = _ints(1000 * D + n_user, n_user, D), _ints(7 * D + n_reps, n_reps, D)
            t_off, t_news, lists = _target_lists(rng, n_user, n_reps)
            valid = (np.arange(n_reps) % 7 != 3).astype(np.uint8)
            ex = rng.integers(0, n_reps, size=(n_user, 7)).astype(np.int32)
            ex[:, 0] = [x[0] if len(x) else -1 for x in lists]
            ex[:, 1], ex[:, 2], ex[:, 6] = -1, n_reps, ex[:, 5]
            gone = sum(int(t % 7 == 3 or t in set(ex[u].tolist())) for u, x in enumerate(lists) for t in x.tolist())
            kw = dict(pad=0, off=0) if D % 4 == 0 and (n_user + n_reps) % 2 else dict(pad=3, off=1)
            ahead = _exact(user, reps, t_off, t_news, **kw)
            assert (ahead >= 0).all()
            ahead = _exact(user, reps, t_off, t_news, valid, ex, **kw)
            assert int((ahead == -1).sum()) == gone and gone >= sum(len(x) > 0 for x in lists)      # at least each user's first target
            total += ahead.size
            minus += gone
    print('D %d: %d targets in 20 shapes, %d of them ineligible by construction' % (D, total, minus))
    assert 0 < minus < total


@pytest.mark.parametrize('n_user,n_reps,per_user', [(64, 257, 40), (5, 600, 600), (70, 1031, 45)])
def test_more_targets_than_the_lds_block_holds(n_user, n_reps, per_user):
    """A user tile with more than 2048 targets: 64 x 40 in one workgroup; 5 x 600 with the news split in two (the counters beyond the block
    live in the workspace); 70 x 45 over two user tiles and four splits, where the first tile overflows and the second does not."""
    from nnr_amd import _lib
    assert min(n_user, 64) * per_user > 2048
    assert (_lib.lib().nnr_pool_rank_workspace_bytes(n_user, n_reps, n_user * per_user) > 0) == (n_reps > 384)
    rng = np.random.default_rng(n_user + n_reps)
    user, reps = _ints(31 + n_user, n_user, 3), _ints(32 + n_reps, n_reps, 3)
    t_off = (np.arange(n_user + 1) * per_user).astype(np.int32)
    t_news = rng.integers(0, n_reps, size=n_user * per_user).astype(np.int32)
    valid = (np.arange(n_reps) % 5 != 2).astype(np.uint8)
    ahead = _exact(user, reps, t_off, t_news, valid)
    assert int((ahead == -1).sum()) == int((t_news % 5 == 2).sum()) > 0
    _exact(user, reps, t_off, t_news, pad=1, off=0)


def test_long_news_ranges_and_users_without_targets():
    """70 001 news: 256 splits of two or three tiles and a merge over 256 partial counts; only the last of five users has targets."""
    user, reps = _ints(5, 5, 3), _ints(6, 70001, 3)
    t_off = np.array([0, 0, 0, 0, 0, 4], dtype=np.int32)
    ahead = _exact(user, reps, t_off, np.array([0, 70000, 35000, 70000], dtype=np.int32))
    assert ahead[1] == ahead[3]


# ------------------------------------------------------------------------------------------------------------------ 2. random inputs
@functools.lru_cache(maxsize=None)
def _normal(D):
    """(user [70, D], reps [3000, D]): drawn once per D, then only read."""
    rng = np.random.default_rng(40 + D)
    user, reps = rng.standard_normal((70, D)).astype(np.float32), rng.standard_normal((3000, D)).astype(np.float32)
    for a in (user, reps):
        a.setflags(write=False)
    return user, reps


@pytest.mark.parametrize('D', [100, 500])
def test_same_bits_as_the_top_k_launch(D):
    """K = 64 and each user's targets = the rows ops.topk_scores returned: ahead is the position in the list and t_score has the list's
    bits.  With 30 random targets per user: ahead < 64 exactly when the target is in the list.  16-byte loads (pad 0) and 4-byte loads
    (stride D + 3, off by one float); both launches split the news, so the merge is on the path."""
    from nnr_amd import ops
    user, reps = _normal(D)
    n_user, K = 70, 64
    rng = np.random.default_rng(D)
    rand = rng.integers(0, 3000, size=(n_user, 30)).astype(np.int32)
    for pad, off in ((0, 0), (3, 1)):
        u_dev, r_dev = _place(user, pad, off), _place(reps, pad + 2 if pad else 0, off)
        idx, sc = ops.topk_scores(u_dev, r_dev, K)
        t_off = torch.arange(n_user + 1, device='cuda', dtype=torch.int32) * K
        ahead, score, pool = ops.pool_ranks(u_dev, r_dev, t_off, idx.reshape(-1).contiguous())
        assert torch.equal(ahead.view(n_user, K), torch.arange(K, device='cuda', dtype=torch.int32).expand(n_user, K))
        assert torch.equal(score.view(n_user, K).view(torch.int32), sc.view(torch.int32))
        assert bool((pool == 3000).all())
        t_off = torch.arange(n_user + 1, device='cuda', dtype=torch.int32) * 30
        ahead, score, _ = ops.pool_ranks(u_dev, r_dev, t_off, _dev(rand.reshape(-1), np.int32))
        ahead, idx_h = ahead.view(n_user, 30).cpu().numpy(), idx.cpu().numpy()
        listed = np.array([[t in set(idx_h[u].tolist()) for t in rand[u]] for u in range(n_user)])
        assert ((ahead < K) == listed).all() and (ahead >= 0).all()
        hit = np.nonzero(listed)
        assert (idx_h[hit[0], ahead[hit]] == rand[hit]).all()
        chain = R.fma_chain32(user[:4], reps)                                    # the header's chain on the host, for four users' targets
        got = score.view(n_user, 30)[:4].cpu().numpy()
        assert (got.view(np.uint32) == np.take_along_axis(chain, rand[:4].astype(np.int64), axis=1).view(np.uint32)).all()
        print('D %d pad %d off %d: %d of %d random targets inside the top %d' % (D, pad, off, int(listed.sum()), listed.size, K))


def test_outputs_do_not_depend_on_the_launch_shape():
    """Three users with 0, 70 and 9 targets against 6 000 news (D = 100): alone (23 news splits and the merge); at rows 62..64 of a 200-user
    launch (the same splits, another place in the tile, across two user tiles and two waves); and at rows 1000.. of a launch of 131 100 user
    rows, which has enough user tiles of its own and does not split.  ahead, t_score and pool_size are the same bits in all three."""
    from nnr_amd import ops, _lib
    D, n_reps = 100, 6000
    g = torch.Generator(device='cuda').manual_seed(3)
    reps = torch.randn((n_reps, D), device='cuda', generator=g)
    users = torch.randn((3, D), device='cuda', generator=g)
    rng = np.random.default_rng(4)
    counts = [0, 70, 9]
    t_news = _dev(rng.integers(0, n_reps, size=sum(counts)), np.int32)
    valid = _dev(np.arange(n_reps) % 11 != 0, np.uint8)
    ex3 = _dev(rng.integers(0, n_reps, size=(3, 20)), np.int32)
    q = _lib.lib().nnr_pool_rank_workspace_bytes
    assert q(3, n_reps, 79) == 4 * 82 * 23 and q(200, n_reps, 79) == 4 * 279 * 23 and q(131100, n_reps, 79) == 0
    outs = []
    for n_user, at in ((3, 0), (200, 62), (131100, 1000)):
        table = torch.randn((n_user, D), device='cuda', generator=g)
        table[at:at + 3] = users
        ex = torch.randint(0, n_reps, (n_user, 20), device='cuda', generator=g, dtype=torch.int32)
        ex[at:at + 3] = ex3
        per = torch.zeros(n_user, dtype=torch.int64)
        per[at:at + 3] = torch.tensor(counts)
        t_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(per, 0)]).to(torch.int32).cuda()
        ahead, score, pool = ops.pool_ranks(table, reps, t_off, t_news, valid=valid, exclude=ex)
        outs.append((ahead.cpu(), score.view(torch.int32).cpu(), pool[at:at + 3].cpu()))
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    assert int(outs[0][2].min()) >= n_reps - 546 - 20 and int((outs[0][0] >= 0).sum()) > 60


@pytest.mark.parametrize('D', [100, 500])
def test_normal_inputs_against_float64(D):
    """20 random targets per user (70 users, 3 000 news), a pool mask and exclusion lists that hold some of the targets: pool_size is exact,
    the -1 entries are exactly the ineligible targets, and every other count lies in pool_rank_ref.bracket."""
    user, reps = _normal(D)
    rng = np.random.default_rng(D + 1)
    t_news = rng.integers(0, 3000, size=(70, 20)).astype(np.int32)
    t_off = (np.arange(71) * 20).astype(np.int32)
    valid = (rng.random(3000) < 0.9).astype(np.uint8)
    ex = rng.integers(0, 3000, size=(70, 12)).astype(np.int32)
    ex[:, 0] = t_news[:, 3]
    el = R.eligible(70, 3000, valid, ex)
    lo, hi = P.bracket(user, reps, el, t_off, t_news.reshape(-1))
    for pad, off in ((0, 0), (3, 1)):
        ahead, score, pool = _run(user, reps, t_off, t_news.reshape(-1), valid, ex, pad=pad, off=off)
        np.testing.assert_array_equal(pool, el.sum(axis=1))
        gone = ~el[np.repeat(np.arange(70), 20), t_news.reshape(-1)]
        assert ((ahead == -1) == gone).all() and gone.sum() >= 70
        ok = ~gone
        assert (lo[ok] <= ahead[ok]).all() and (ahead[ok] <= hi[ok]).all(), int(((lo > ahead) | (ahead > hi))[ok].sum())
        exact = P.ranks(R.scores64(user, reps), el, t_off, t_news.reshape(-1))[0]
        print('D %d pad %d off %d: %d targets, widest bracket %d, %d counts differ from float64\'s' %
              (D, pad, off, int(ok.sum()), int((hi - lo)[ok].max()), int((ahead != exact)[ok].sum())))


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
@functools.lru_cache(maxsize=None)
def _split():
    """The synthetic split of tests/test_hip_recommend_gpu.py: 300 news with short titles, 40 behaviours over 25 distinct (user, history) rows."""
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


def _agrees_with_recommend(E, model, dc, rows, targets, ahead, pool_size, **kw):
    """ahead < 10 exactly when the target is in the row's recommend(K = 10) list, and then at that position; with a pool of at most 64 news,
    pool_size is the length of the row's whole list."""
    news_i, _ = E.recommend(model, dc, 10, rows=rows, **kw)
    news_i, a, t = news_i.cpu().numpy(), ahead.cpu().numpy(), targets.cpu().numpy()
    for i in range(len(t)):
        where = np.nonzero(news_i[i] == t[i])[0]
        assert (where.size == 1 and where[0] == a[i]) if 0 <= a[i] < 10 else where.size == 0, (i, a[i], where)
    if 'pool' in kw:
        full, _ = E.recommend(model, dc, 64, rows=rows, **kw)
        assert torch.equal((full >= 0).sum(dim=1).to(torch.int32), pool_size)


@pytest.mark.parametrize('news,user', [('CNN', 'ATT'), ('MHSA', 'MHSA'), ('CNN', 'PUE')])
def test_rank_in_pool_end_to_end(news, user):
    from nnr_amd import evaluate as E
    dc, _ = _split()
    model = _e2e_model(news, user)
    t = dc.t
    hist, hmask = t['beh_history'].cpu().numpy().astype(np.int64), t['beh_history_mask'].cpu().numpy() != 0
    labels = (np.random.default_rng(5).random(40) < 0.6).astype(np.int64)
    rows, targets = E.clicked_targets(dc, labels)
    assert rows.dtype == targets.dtype == torch.int64 and rows.cpu().tolist() == np.nonzero(labels)[0].tolist()
    assert torch.equal(targets, dc.samples[rows, 0].long()) and 15 <= rows.numel() < 40

    # the whole default pool
    E.LAST_STATS.clear()
    ahead, pool_size, m = E.rank_in_pool(model, dc, rows, targets)
    st = dict(E.LAST_STATS)
    R_ = rows.numel()
    assert model.training and ahead.dtype == pool_size.dtype == torch.int32 and tuple(ahead.shape) == tuple(pool_size.shape) == (R_,)
    assert ahead.is_cuda and pool_size.is_cuda
    assert st['mode'] == 'rank_in_pool' and st['rows'] == R_ and st['targets'] == R_ and st['pool'] == 299 and 1 <= st['user_rows'] <= 25
    want = P.metrics(ahead.cpu().numpy(), pool_size.cpu().numpy())
    assert set(m) == set(want) and m['counted'] == want['counted'] and m['skipped'] == want['skipped'] == int((ahead < 0).sum())
    for k in want:
        assert m[k] == pytest.approx(want[k], rel=1e-13), k
    _agrees_with_recommend(E, model, dc, rows, targets, ahead, pool_size)
    live = np.array([int(hmask[r].sum()) for r in rows.cpu().numpy()])
    distinct_live = np.array([len(set(hist[r][hmask[r]].tolist())) for r in rows.cpu().numpy()])
    assert (pool_size.cpu().numpy() == 299 - distinct_live).all() and live.max() > 0
    a2, p2, m2 = E.rank_in_pool(model, dc, rows, targets, dedup_users=False)
    assert torch.equal(a2, ahead) and torch.equal(p2, pool_size) and m2 == m and E.LAST_STATS['user_rows'] == R_
    a3, p3, m3 = E.rank_in_pool(model, dc, rows, targets, ks=(1, 3), batch_size=7)
    assert torch.equal(a3, ahead) and set(m3) == {'counted', 'skipped', 'hr@1', 'ndcg@1', 'hr@3', 'ndcg@3', 'mrr', 'percentile'}
    assert m3['hr@1'] == m3['ndcg@1'] == float((ahead == 0).sum()) / m['counted']

    # a clicked news that stands in its own row's history; a target outside the pool; a repeated row
    r_h = int(np.argmax(hmask.sum(axis=1)))
    in_hist = int(hist[r_h][hmask[r_h]][0])
    pool = np.unique(np.concatenate([np.random.default_rng(2).choice(np.arange(1, 300), size=50, replace=False), [in_hist]]))
    outside = int(np.setdiff1d(np.arange(1, 300), np.concatenate([pool, hist[0][hmask[0]]]))[0])
    inside = [int(v) for v in pool if v not in set(hist[5][hmask[5]].tolist())][:2]
    free = [int(v) for v in pool if v not in set(hist[r_h][hmask[r_h]].tolist())][-1]
    rows2, targets2 = [r_h, 0, 5, 5, r_h], [in_hist, outside, inside[0], inside[1], free]
    res = {}
    for ex in (True, False):
        a, p, mm = E.rank_in_pool(model, dc, rows2, targets2, pool=pool, exclude_history=ex)
        res[ex] = a.cpu().tolist()
        assert a[1] == -1 and (a[0] == -1) == ex and min(res[ex][2:]) >= 0 and res[ex][2] != res[ex][3] and p[0] == p[4] and p[2] == p[3]
        assert mm['skipped'] == (2 if ex else 1) and mm['counted'] + mm['skipped'] == 5
        _agrees_with_recommend(E, model, dc, torch.tensor(rows2), torch.tensor(targets2), a, p, pool=pool, exclude_history=ex)
        ad, pd, _ = E.rank_in_pool(model, dc, rows2, targets2, pool=pool, exclude_history=ex, dedup_users=False)
        assert torch.equal(ad, a) and torch.equal(pd, p)
    assert res[False][0] >= 0
    everything_skipped = E.rank_in_pool(model, dc, [0, 0], [outside, outside], pool=pool)[2]
    assert everything_skipped['counted'] == 0 and np.isnan(everything_skipped['mrr']) and np.isnan(everything_skipped['percentile'])
    with pytest.raises(ValueError, match='targets'):
        E.rank_in_pool(model, dc, [0, 1], [300, 1])
    with pytest.raises(ValueError, match='one target per entry'):
        E.rank_in_pool(model, dc, [0, 1], [1])
    with pytest.raises(ValueError, match='rows'):
        E.rank_in_pool(model, dc, [40], [1])
    print('%s+%s: %d clicked rows, metrics %r' % (news, user, R_, m))
