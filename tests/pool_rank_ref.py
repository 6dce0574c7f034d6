"""Restatement of nnr_pool_ranks (include/nnr_hip.h) for the tests, in numpy float64 and integers, over recommend_ref's scores and
eligibility: ahead[j] = the eligible rows that precede target j of its user (greater score, or equal score and smaller row), -1 for a target
that is itself ineligible; pool_size[u] = the user's eligible rows; the full-ranking metrics of evaluate.rank_in_pool from `ahead`; and
the bracket that judges a float32 count against float64 without asking for its bits."""
import math

import numpy as np

import recommend_ref as R


def _user_of(t_off):
    """The user row of every target: user u owns entries t_off[u] .. t_off[u + 1] - 1."""
    t_off = np.asarray(t_off, dtype=np.int64)
    return np.repeat(np.arange(t_off.size - 1), np.diff(t_off))


def ranks(scores, el, t_off, t_news):
    """(ahead int32 [T], pool_size int32 [n_user]) by brute force over `scores` [n_user, n_reps] and the eligibility `el` (bool, same shape)."""
    t_news = np.asarray(t_news, dtype=np.int64)
    n_user, n_reps = scores.shape
    ahead = np.empty(t_news.size, dtype=np.int32)
    rows = np.arange(n_reps)
    for j, (u, t) in enumerate(zip(_user_of(t_off), t_news)):
        before = (scores[u] > scores[u, t]) | ((scores[u] == scores[u, t]) & (rows < t))
        ahead[j] = int((before & el[u]).sum()) if el[u, t] else -1
    return ahead, el.sum(axis=1).astype(np.int32)


def ranks_naive(user, reps, t_off, t_news, valid=None, exclude=None):
    """The contract as loops over plain Python numbers (tiny cases only)."""
    n_user, n_reps, D = len(user), len(reps), len(user[0])
    ahead, pool = [], []
    for u in range(n_user):
        banned = set(int(r) for r in exclude[u]) if exclude is not None else set()
        ok = [(valid is None or valid[r] != 0) and r not in banned for r in range(n_reps)]
        sc = [sum(float(user[u][d]) * float(reps[r][d]) for d in range(D)) for r in range(n_reps)]
        pool.append(sum(ok))
        for j in range(int(t_off[u]), int(t_off[u + 1])):
            t = int(t_news[j])
            if not ok[t]:
                ahead.append(-1)
                continue
            n = 0
            for r in range(n_reps):
                if ok[r] and (sc[r] > sc[t] or (sc[r] == sc[t] and r < t)):
                    n += 1
            ahead.append(n)
    return np.asarray(ahead, dtype=np.int32).reshape(-1), np.asarray(pool, dtype=np.int32)


def metrics(ahead, pool_size, ks=(5, 10)):
    """evaluate.rank_in_pool's metrics from `ahead` and the per-target `pool_size`, one target at a time in Python floats: over the counted
    targets (ahead >= 0)  hr@k = mean[ahead < k],  ndcg@k = mean[ahead < k ? 1 / log2(ahead + 2) : 0],  mrr = mean[1 / (ahead + 1)];
    percentile = mean[1 - ahead / (pool_size - 1)] over the counted ones with pool_size > 1.  A mean over nothing is NaN."""
    ahead, pool_size = [int(a) for a in ahead], [int(p) for p in pool_size]
    kept = [(a, p) for a, p in zip(ahead, pool_size) if a >= 0]
    mean = lambda xs: math.fsum(xs) / len(xs) if xs else float('nan')
    out = {'counted': len(kept), 'skipped': len(ahead) - len(kept)}
    for k in ks:
        out['hr@%d' % k] = mean([1.0 if a < k else 0.0 for a, _ in kept])
        out['ndcg@%d' % k] = mean([1.0 / math.log2(a + 2) if a < k else 0.0 for a, _ in kept])
    out['mrr'] = mean([1.0 / (a + 1) for a, _ in kept])
    out['percentile'] = mean([1.0 - a / (p - 1) for a, p in kept if p > 1])
    return out


def bracket(user, reps, el, t_off, t_news):
    """(lo, hi) int64 [T] for targets that are eligible (-1 / -1 for the others): with s64 the float64 scores and b = recommend_ref.bound,
    a float32 chain's score lies within b of s64 for either row, so a row whose float64 score exceeds the target's by more than the two
    bounds added precedes it in float32 whatever the rounding did, and a row that is below it by more than that cannot:
      lo = #{eligible r: s64(u, r) > s64(u, t) + b(u, r) + b(u, t)}  <=  ahead  <=  hi = #{eligible r != t: s64(u, r) >= s64(u, t) - b(u, r) - b(u, t)}.
    (The two bounds added is recommend_ref.band_check's margin; b already carries a factor 2 of slack.  The target itself never precedes
    itself; leaving it out of hi only tightens the bracket.)"""
    s64, b = R.scores64(user, reps), R.bound(user, reps)
    t_news = np.asarray(t_news, dtype=np.int64)
    lo, hi = np.full(t_news.size, -1, dtype=np.int64), np.full(t_news.size, -1, dtype=np.int64)
    for j, (u, t) in enumerate(zip(_user_of(t_off), t_news)):
        if not el[u, t]:
            continue
        room = b[u] + b[u, t]
        others = el[u].copy()
        others[t] = False
        lo[j] = int((el[u] & (s64[u] > s64[u, t] + room)).sum())
        hi[j] = int((others & (s64[u] >= s64[u, t] - room)).sum())
    return lo, hi
