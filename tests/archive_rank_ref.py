"""Restatement of nnr_topk_archive_scores / nnr_pool_archive_ranks (include/nnr_hip.h) for the tests, in numpy float64, on top of
recommend_ref (eligibility, order, the fmaf chain) and pool_rank_ref (ranks): a user is A vectors and the score of a pair is

    s_a = <user[u, a], reps[r]>,   score = sum_a w_a s_a,   w = softmax_a(scale * s_a).

The band of a float32 result around the float64 score:

    B(u, r) = (1 + |scale| * (max_a s_a - min_a s_a)) * max_a b_a(u, r)  +  2^-17 * max_a |s_a|

b_a = recommend_ref.bound of archive a (D * 2^-23 * sum_d |u_d r_d|, the bound of its fp32 chain).  First term: the score moves by at most
w_j (1 + |scale| spread) per unit of s_j (d score / d s_j = w_j (1 + scale (s_j - score)), and |s_j - score| <= spread), and the w_j add up
to 1.  Second term: the weights and the weighted sums are a few dozen fp32 roundings (the exponential's 2 ulp and the rounding of its
argument, one rounding per update of den and num, the division); an error eps_a of weight a moves the score by eps_a w_a (s_a - score),
at most max_a eps_a * spread <= 2 max_a eps_a * max_a |s_a|, and 2^-17 = 64 * 2^-23 leaves room for 32 such roundings of 2^-24 doubled.
combine32 is the header's operation sequence in numpy float32 (np.exp for expf: the same function to 1 ulp, not the same bits), which
tests/test_archive_rank_host.py holds against the band."""
import numpy as np

import pool_rank_ref as P
import recommend_ref as R

eligible, topk, ranks = R.eligible, R.topk, P.ranks


def as_archives(user, A=None):
    """`user` as [n_user, A, D]: given so, or as [n_user, A * D]."""
    user = np.asarray(user)
    return user if user.ndim == 3 else user.reshape(user.shape[0], A, -1)


def chains64(user, reps):
    """s_a [n_user, A, n_reps] float64."""
    user = np.asarray(user)
    return np.stack([R.scores64(user[:, a], reps) for a in range(user.shape[1])], axis=1)


def combine64(s, scale):
    """sum_a w_a s_a with w = softmax_a(scale * s_a) over axis 1 of s [n_user, A, n_reps], float64."""
    z = scale * s
    w = np.exp(z - z.max(axis=1, keepdims=True))
    return (w * s).sum(axis=1) / w.sum(axis=1)


def scores64(user, reps, scale):
    """[n_user, n_reps] float64 combined scores of user [n_user, A, D]."""
    return combine64(chains64(user, reps), float(scale))


def band(user, reps, scale):
    """B [n_user, n_reps] of the module's docstring."""
    user = np.asarray(user)
    s = chains64(user, reps)
    b = np.stack([R.bound(user[:, a], reps) for a in range(user.shape[1])], axis=1)
    return (1.0 + abs(float(scale)) * (s.max(axis=1) - s.min(axis=1))) * b.max(axis=1) + 2.0 ** -17 * np.abs(s).max(axis=1)


def combine32(s, scale):
    """The header's combine in float32, one operation at a time: s float32 [..., A] -> [...]."""
    s = np.asarray(s, dtype=np.float32)
    scale = np.float32(scale)
    one = np.ones(s.shape[:-1], dtype=np.float32)
    m, den, num = s[..., 0].copy(), one.copy(), s[..., 0].copy()
    for a in range(1, s.shape[-1]):
        x = s[..., a]
        up = (x < m) if scale < 0 else (x > m)
        e = np.exp((scale * np.where(up, m - x, x - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
        den = R.fma32(np.where(up, den, one), e, np.where(up, one, den))
        num = R.fma32(np.where(up, num, x), e, np.where(up, x, num))
        m = np.where(up, x, m)
    return (num / den).astype(np.float32)


def scores32(user, reps, scale):
    """[n_user, n_reps] float32: the fmaf chain of every archive (recommend_ref.fma_chain32), combined by combine32."""
    user = np.asarray(user, dtype=np.float32)
    s = np.stack([R.fma_chain32(user[:, a], reps) for a in range(user.shape[1])], axis=-1)
    return combine32(s, scale)


def band_check(s64, b, el, K, idx, score):
    """recommend_ref.band_check for given float64 scores s64 and band b [n_user, n_reps]: every returned score within b of s64; distinct
    eligible rows sorted by their OWN scores descending, equal scores by ascending row, -1 / -inf behind; no eligible row left out whose s64
    exceeds the K-th returned one's by more than the two bands added; a short list holds every eligible row.  Returns the two worst ratios."""
    worst_a = worst_c = 0.0
    for u in range(s64.shape[0]):
        got = idx[u]
        n = int((got >= 0).sum())
        rows = got[:n].astype(np.int64)
        assert (got[n:] == -1).all() and np.isneginf(score[u, n:]).all(), (u, 'tail')
        assert n == min(K, int(el[u].sum())), (u, 'length', n)
        assert len(set(rows.tolist())) == n and el[u, rows].all(), (u, 'distinct eligible rows')
        sc = score[u, :n]
        assert np.isfinite(sc).all(), (u, 'finite')
        assert ((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (rows[:-1] < rows[1:]))).all(), (u, 'order')
        err = np.abs(sc.astype(np.float64) - s64[u, rows])
        assert (err <= b[u, rows]).all(), (u, 'score', float((err / b[u, rows]).max()))
        if n:
            worst_a = max(worst_a, float((err / np.maximum(b[u, rows], 1e-300)).max()))
        out = el[u].copy()
        out[rows] = False
        if out.any():
            assert n == K, (u, 'an eligible row is missing from a short list')
            last = rows[-1]
            excess = s64[u, out] - s64[u, last]
            room = b[u, out] + b[u, last]
            assert (excess <= room).all(), (u, 'omitted', float((excess - room).max()))
            worst_c = max(worst_c, float((excess / np.maximum(room, 1e-300)).max()))
    return worst_a, worst_c


def bracket(s64, b, el, t_off, t_news):
    """pool_rank_ref.bracket for given float64 scores and band: (lo, hi) int64 [T], -1 / -1 for ineligible targets."""
    t_news = np.asarray(t_news, dtype=np.int64)
    lo, hi = np.full(t_news.size, -1, dtype=np.int64), np.full(t_news.size, -1, dtype=np.int64)
    for j, (u, t) in enumerate(zip(P._user_of(t_off), t_news)):
        if not el[u, t]:
            continue
        room = b[u] + b[u, t]
        others = el[u].copy()
        others[t] = False
        lo[j] = int((el[u] & (s64[u] > s64[u, t] + room)).sum())
        hi[j] = int((others & (s64[u] >= s64[u, t] - room)).sum())
    return lo, hi
