"""Restatement of nnr_list_scores (include/nnr_hip.h) for the tests: scores[j] = sum_d user[row[j], d] * reps[cand[j], d], in the dtype
asked for (float64: the expectation; float32: the same formula at the kernel's precision, whose error sets the kernel's bar)."""
import numpy as np


def list_scores(user, reps, row, cand, dtype=np.float64):
    """user [n_user, D], reps [n_reps, D], row / cand integer [n] -> [n] in `dtype` (products and sums taken in `dtype`)."""
    u = np.asarray(user, dtype=dtype)[np.asarray(row, dtype=np.int64)]
    r = np.asarray(reps, dtype=dtype)[np.asarray(cand, dtype=np.int64)]
    return (u * r).sum(axis=1, dtype=dtype)


def list_scores_naive(user, reps, row, cand):
    """The formula as a double loop over samples and columns, float64."""
    out = np.zeros(len(row), dtype=np.float64)
    for j in range(len(row)):
        for d in range(np.shape(user)[1]):
            out[j] += float(user[row[j]][d]) * float(reps[cand[j]][d])
    return out


def tables(n_user, n_reps, D, n, ldu, ldr, seed):
    """Random op-level inputs: float32 buffers [n_user, ldu] / [n_reps, ldr] (the tables are their first D columns, the rest NaN so that a read
    past a row's width shows), indices that repeat when the tables are small."""
    rng = np.random.default_rng(seed)
    ub = np.full((n_user, ldu), np.nan, dtype=np.float32)
    rb = np.full((n_reps, ldr), np.nan, dtype=np.float32)
    ub[:, :D] = rng.standard_normal((n_user, D), dtype=np.float32)
    rb[:, :D] = rng.standard_normal((n_reps, D), dtype=np.float32)
    row = rng.integers(0, n_user, size=n).astype(np.int32)
    cand = rng.integers(0, n_reps, size=n).astype(np.int32)
    return ub, rb, row, cand
