"""numpy restatement of the device negative sampler (nnr_negative_sample; the construction is stated at its declaration in
include/nnr_hip.h and followed here line by line).  Bit-exact by construction: 32-bit integer arithmetic only.  Imports nothing from
nnr_amd: the contract is that this file and the kernel agree bit for bit."""
import numpy as np

GOLDEN = 0x9E3779B9
_M32 = np.uint64(0xFFFFFFFF)


def hash32(x):
    """nnr_hash32 (csrc/common.h): the lowbias32 finaliser, on uint32 arrays (computed in uint64, masked after every product)."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & _M32
    x ^= x >> np.uint64(16)
    return x


def key_of(seed, epoch):
    """key = H(seed ^ H(epoch + 0x9E3779B9))"""
    return hash32(np.uint64(int(seed) & 0xFFFFFFFF) ^ hash32(np.uint64((int(epoch) + GOLDEN) & 0xFFFFFFFF)))


def draws(beh, K, seed, epoch):
    """r[:, j] = H(H(b ^ key) + j * 0x9E3779B9 + 1) for the behaviours `beh`: uint64 [len(beh), K] holding 32-bit values."""
    h = hash32(np.asarray(beh, dtype=np.uint64) ^ key_of(seed, epoch))
    j = np.arange(K, dtype=np.uint64)
    return hash32((h[:, None] + j[None, :] * np.uint64(GOLDEN) + np.uint64(1)) & _M32)


def positions(beh, m, K, seed, epoch):
    """Positions [len(beh), K] (int64) that the sampler reads in a list of length m[i] of behaviour beh[i].
    m <= K: j % m.  m > K: the partial Fisher-Yates walk over the virtual array a[p] = p -- for j = 0 .. K - 1: p = j + ((r_j * (m - j)) >> 32),
    read a[p], then a[p] = a[j]; (pos[t], val[t]) is the entry step t displaced, pos[t] < 0: none."""
    beh = np.asarray(beh, dtype=np.int64)
    m = np.broadcast_to(np.asarray(m, dtype=np.int64), beh.shape)
    n = beh.shape[0]
    out = np.arange(K, dtype=np.int64)[None, :] % m[:, None]
    rnd = m > K
    if not rnd.any():
        return out
    r = draws(beh, K, seed, epoch)
    pos = np.full((K, n), -1, dtype=np.int64)
    val = np.zeros((K, n), dtype=np.int64)
    for j in range(K):
        span = np.maximum(m - j, 0).astype(np.uint64)
        p = j + ((r[:, j] * span) >> np.uint64(32)).astype(np.int64)
        ap, aj, hit = p.copy(), np.full(n, j, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        for t in range(j):
            at_p, at_j = pos[t] == p, pos[t] == j
            ap[at_p], hit[at_p] = val[t][at_p], t
            aj[at_j] = val[t][at_j]
        for t in range(j):
            sel = hit == t
            val[t][sel] = aj[sel]
        pos[j] = np.where(hit < 0, p, -1)
        val[j] = aj
        out[rnd, j] = ap[rnd]
    return out


def sample(clicks, neg_offsets, neg_ids, K, seed, epoch, beh_idx=None):
    """Rows [len(beh_idx), 1 + K] int32 of the sample table: column 0 the click, then the sampled non-clicks."""
    clicks, neg_offsets, neg_ids = np.asarray(clicks), np.asarray(neg_offsets, dtype=np.int64), np.asarray(neg_ids)
    beh = np.arange(clicks.shape[0], dtype=np.int64) if beh_idx is None else np.asarray(beh_idx, dtype=np.int64)
    m = neg_offsets[beh + 1] - neg_offsets[beh]
    assert (m > 0).all()
    out = np.empty((beh.shape[0], 1 + K), dtype=np.int32)
    out[:, 0] = clicks[beh]
    out[:, 1:] = neg_ids[neg_offsets[beh][:, None] + positions(beh, m, K, seed, epoch)]
    return out


def csr(behaviors):
    """[(click, [non-clicks]), ...] -> (clicks int32, neg_offsets int64, neg_ids int32)."""
    clicks = np.asarray([c for c, _ in behaviors], dtype=np.int32)
    off = np.zeros(len(behaviors) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(n) for _, n in behaviors])
    return clicks, off, np.asarray([v for _, n in behaviors for v in n], dtype=np.int32)
