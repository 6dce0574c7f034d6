"""Restatement of nnr_cne_pair_triples (include/nnr_hip.h) for the tests, in numpy: the reference scores dev samples in batches of `batch_size`
consecutive samples (the last one short) and runs two encoder calls per batch of b samples -- the candidate call over b sequences, the history
call over b * H sequences, sequence s * H + h.  Inside a call the sequences are ranked by title length and by content length, descending, equal
lengths in ascending sequence index; pc(i) = order_c[rank_t[i]] is the sequence whose content memory gates title i, pt(i) = order_t[rank_c[i]]
the one whose title memory gates content i.  The ranking is the definition itself, by brute force: rank(i) = #(longer) + #(equal and earlier)."""
import numpy as np


def stable_desc_rank(lengths):
    """rank[i] = sorted position of sequence i: the sequences longer than i, plus the equally long ones in front of it."""
    l = np.asarray(lengths, dtype=np.int64)
    i = np.arange(l.size)
    ahead = (l[None, :] > l[:, None]) | ((l[None, :] == l[:, None]) & (i[None, :] < i[:, None]))
    return ahead.sum(axis=1)


def call_partners(tl, cl):
    """(pc, pt) of one call from its sequences' title / content lengths: sequence indices inside the call."""
    rank_t, rank_c = stable_desc_rank(tl), stable_desc_rank(cl)
    order_t, order_c = np.empty_like(rank_t), np.empty_like(rank_c)
    order_t[rank_t] = np.arange(rank_t.size)
    order_c[rank_c] = np.arange(rank_c.size)
    return order_c[rank_t], order_t[rank_c]


def pair_triples(hist, cand, tlen, clen, batch_size, first=0, count=None):
    """-> (pc_hist, pt_hist) int32 [count, H], (pc_cand, pt_cand) int32 [count]: partner NEWS of every history slot / candidate of the samples
    first .. first + count - 1, batch by batch (whole batches: first is a multiple of batch_size, the range ends at one or with the split)."""
    hist, cand = np.asarray(hist), np.asarray(cand).reshape(-1)
    n, H = hist.shape
    count = n - first if count is None else count
    assert first % batch_size == 0 and 0 <= first and first + count <= n and (first + count == n or count % batch_size == 0)
    pc_h, pt_h = np.empty((count, H), dtype=np.int32), np.empty((count, H), dtype=np.int32)
    pc_c, pt_c = np.empty(count, dtype=np.int32), np.empty(count, dtype=np.int32)
    for s in range(0, count, batch_size):
        e = min(s + batch_size, count)
        ids = hist[first + s:first + e].reshape(-1)
        pc, pt = call_partners(tlen[ids], clen[ids])
        pc_h[s:e], pt_h[s:e] = ids[pc].reshape(e - s, H), ids[pt].reshape(e - s, H)
        ids = cand[first + s:first + e]
        pc, pt = call_partners(tlen[ids], clen[ids])
        pc_c[s:e], pt_c[s:e] = ids[pc], ids[pt]
    return pc_h, pt_h, pc_c, pt_c


def distinct_triples(hist, cand, tlen, clen, batch_size, window):
    """How many (news, partner, partner) triples an evaluation in windows of `window` batches encodes: the distinct ones of every window."""
    hist, cand = np.asarray(hist), np.asarray(cand).reshape(-1)
    n, total = hist.shape[0], 0
    for w0 in range(0, n, window * batch_size):
        cnt = min(window * batch_size, n - w0)
        pc_h, pt_h, pc_c, pt_c = pair_triples(hist, cand, tlen, clen, batch_size, w0, cnt)
        own = np.concatenate([hist[w0:w0 + cnt].reshape(-1), cand[w0:w0 + cnt]])
        rows = np.stack([own, np.concatenate([pc_h.reshape(-1), pc_c]), np.concatenate([pt_h.reshape(-1), pt_c])], axis=1)
        total += np.unique(rows, axis=0).shape[0]
    return total


def mask_lengths(mask):
    """Ones of every mask row with position 0 forced to 1 (newsEncoders.py:108-109)."""
    m = np.asarray(mask) != 0
    return (m.sum(axis=1) + ~m[:, 0]).astype(np.int32)
