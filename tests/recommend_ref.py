"""Restatement of nnr_topk_scores (include/nnr_hip.h) for the tests, in numpy float64: eligibility, the order (score descending, equal
scores by ascending row, ties at the cut the same way), short pools (idx = -1, score = -inf), and the band check that judges a float32
result against float64 without asking for its bits."""
import numpy as np


def scores64(user, reps):
    """[n_user, n_reps] float64 inner products."""
    return np.asarray(user, dtype=np.float64) @ np.asarray(reps, dtype=np.float64).T


def eligible(n_user, n_reps, valid=None, exclude=None):
    """bool [n_user, n_reps]: row r is eligible for user u when valid is None or valid[r] != 0, and r is not in exclude[u] (entries outside
    0 .. n_reps - 1 are ignored, duplicates allowed)."""
    el = np.ones((n_user, n_reps), dtype=bool)
    if valid is not None:
        el &= (np.asarray(valid).reshape(1, n_reps) != 0)
    if exclude is not None:
        ex = np.asarray(exclude).reshape(n_user, -1).astype(np.int64)
        u, e = np.nonzero((ex >= 0) & (ex < n_reps))
        el[u, ex[u, e]] = False
    return el


def topk(scores, el, K):
    """(idx int32 [n_user, K], score [n_user, K] in scores' dtype) of the eligible entries of `scores` [n_user, n_reps]."""
    n_user, n_reps = scores.shape
    idx = np.full((n_user, K), -1, dtype=np.int32)
    out = np.full((n_user, K), -np.inf, dtype=scores.dtype)
    for u in range(n_user):
        rows = np.nonzero(el[u])[0]
        order = rows[np.argsort(-scores[u, rows], kind='stable')][:K]        # stable: equal scores stay in ascending row order
        idx[u, :order.size] = order
        out[u, :order.size] = scores[u, order]
    return idx, out


def topk_naive(user, reps, K, valid=None, exclude=None):
    """The contract as loops over plain Python numbers (tiny cases only): K rounds of 'the best eligible row not taken yet'."""
    n_user, n_reps, D = len(user), len(reps), len(user[0])
    idx, out = [], []
    for u in range(n_user):
        banned = set(int(r) for r in exclude[u]) if exclude is not None else set()
        cand = []
        for r in range(n_reps):
            if (valid is None or valid[r] != 0) and r not in banned:
                cand.append((sum(float(user[u][d]) * float(reps[r][d]) for d in range(D)), r))
        ri, rs = [], []
        for _ in range(K):
            best = None
            for s, r in cand:
                if r not in ri and (best is None or s > best[0] or (s == best[0] and r < best[1])):
                    best = (s, r)
            ri.append(-1 if best is None else best[1])
            rs.append(-np.inf if best is None else best[0])
        idx.append(ri)
        out.append(rs)
    return np.asarray(idx, dtype=np.int32).reshape(n_user, K), np.asarray(out, dtype=np.float64).reshape(n_user, K)


def bound(user, reps):
    """b(u, r) = D * 2^-23 * sum_d |u_d r_d| [n_user, n_reps]: the bound of an fp32 fused-multiply-add sum of D terms in any order (D
    roundings of at most 2^-24 relative each, first order), with a factor 2 of slack."""
    D = np.asarray(user).shape[1]
    return D * 2.0 ** -23 * (np.abs(np.asarray(user, dtype=np.float64)) @ np.abs(np.asarray(reps, dtype=np.float64)).T)


def band_check(user, reps, el, K, idx, score):
    """A float32 result (idx, score) judged by float64, nothing left out; raises AssertionError naming the first violation and returns
    (largest |score - float64| / bound, largest excess of an omitted row over the K-th returned / the two bounds added):
      (a) every returned score is within b of the float64 score of its row;
      (b) the list holds distinct eligible rows, sorted by its OWN scores descending, equal scores by ascending row, -1 / -inf behind;
      (c) no eligible row left out has a float64 score above the K-th returned one's by more than the two rows' bounds added; a list shorter
          than K holds every eligible row."""
    s64, b = scores64(user, reps), bound(user, reps)
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
        assert (err <= b[u, rows]).all(), (u, 'score', float(err.max()))
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


def fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays, ONE rounding (what fmaf does), through float64: the product of two float32 is exact in float64;
    TwoSum gives the float64 sum s and its exact error e; rounding s to float32 is the correct rounding of s + e unless s lies exactly on the
    midpoint of two float32 neighbours and e != 0, in which case e's sign decides.  Finite inputs without overflow."""
    p, c = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)                                                # exact: both are float64 and close
    toward = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    half = (toward.astype(np.float64) - r.astype(np.float64)) / 2
    move = (d != 0) & (d == half) & (np.sign(e) == np.sign(d))                  # on the midpoint, and the exact value is beyond it
    return np.where(move, toward, r).astype(np.float32)


def fma_chain32(user, reps):
    """[n_user, n_reps] float32: acc = fmaf(user[u, d], reps[r, d], acc) over d = 0, 1, .. from +0, the order include/nnr_hip.h states."""
    user, reps = np.asarray(user, dtype=np.float32), np.asarray(reps, dtype=np.float32)
    acc = np.zeros((user.shape[0], reps.shape[0]), dtype=np.float32)
    for d in range(user.shape[1]):
        acc = fma32(user[:, d:d + 1], reps[None, :, d], acc)
    return acc
