#!/usr/bin/env python3
"""Full-pool ranks (profiles/pool_rank_summary.md): the nnr_pool_ranks launch against this build's own nnr_topk_scores launch at the same
shape, and against stock torch, on the same device in the same session.

  python tools/pool_rank_bench.py [--users 50000,64] [--targets 1,8] [--news 42000] [--D 500] [--history 50] [--K 10] [--rounds 5]

Random normal tables, a pool of every row but row 0, `--history` random excluded rows per user (a fifth of the slots are -1 pads), and
`--targets` random targets per user.  One point per (users, targets per user).

The stock form is what a user of stock ops has to write: the user rows in chunks sized so that a chunk's [chunk, news] float32 scores are
one 1 GB block (tools/recommend_bench.py's chunk), per chunk `user[c] @ reps.T`, a masked_fill for the pool, an index-put of -inf for the
history lists, then per target a gather of its score, two comparisons against the block and a row sum; pool_size is one more compare
and sum.

Times: the three forms take turns, `--rounds` rounds after one warm-up call each, every call between two device events; the median and
the minimum per form are reported.  TF = 2 * users * news * D / time against the 157.3 TF fp32 matrix peak.  Bytes: torch's peak allocated
bytes during one call above what was allocated before it; the cached workspace of the fused launches is listed separately.
One JSON line per point on stdout, with the library's build id."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops                                                   # noqa: E402

PEAK_TF = 157.3


def event_ms(fn):
    """(result, milliseconds) of one call of fn() between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return out, start.elapsed_time(end)


def peak_mb(fn):
    """MB that torch's allocator peaked at during fn() above what was allocated before the call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def stock_ranks(user, reps, tn, valid, exclude, block_bytes=1 << 30):
    """The chunked stock-torch form for a fixed number of targets per user (tn int64 [n_user, T]): (ahead int64 [n_user, T] with -1 for an
    ineligible target, pool_size int64 [n_user])."""
    n_user, n_reps = user.shape[0], reps.shape[0]
    chunk = max(1, block_bytes // (4 * n_reps))
    out_ = ~valid.bool() if valid is not None else None
    cols = torch.arange(n_reps, device=user.device).view(1, n_reps)
    ahead = torch.empty(tn.shape, device=user.device, dtype=torch.int64)
    pool = torch.empty(n_user, device=user.device, dtype=torch.int64)
    for s in range(0, n_user, chunk):
        sc = user[s:s + chunk] @ reps.t()
        if out_ is not None:
            sc.masked_fill_(out_, float('-inf'))
        if exclude is not None:
            ex = exclude[s:s + chunk].long()
            live = (ex >= 0) & (ex < n_reps)
            sc.scatter_reduce_(1, torch.where(live, ex, 0), torch.where(live, float('-inf'), float('inf')).to(sc.dtype), 'amin')
        pool[s:s + chunk] = (sc != float('-inf')).sum(dim=1)
        t = tn[s:s + chunk]
        ts = sc.gather(1, t)
        for k in range(t.shape[1]):
            tk, sk = t[:, k:k + 1], ts[:, k:k + 1]
            a = ((sc > sk) | ((sc == sk) & (cols < tk))).sum(dim=1)
            ahead[s:s + chunk, k] = torch.where(sk[:, 0] == float('-inf'), -1, a)
    return ahead, pool


def point(n_user, per_user, a, reps, valid, g):
    user = torch.randn((n_user, a.D), device='cuda', generator=g)
    ex = torch.randint(1, a.news, (n_user, a.history), device='cuda', generator=g, dtype=torch.int32)
    ex[torch.rand((n_user, a.history), device='cuda', generator=g) < 0.2] = -1
    tn = torch.randint(0, a.news, (n_user, per_user), device='cuda', generator=g)
    t_off = (torch.arange(n_user + 1, device='cuda') * per_user).to(torch.int32)
    t_news = tn.reshape(-1).to(torch.int32).contiguous()
    forms = {'pool_ranks': lambda: ops.pool_ranks(user, reps, t_off, t_news, valid=valid, exclude=ex, check=False),
             'topk': lambda: ops.topk_scores(user, reps, a.K, valid=valid, exclude=ex, check=False),
             'stock': lambda: stock_ranks(user, reps, tn, valid, ex)}
    res = {k: f() for k, f in forms.items()}                                    # one warm-up call of every form
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.rounds):                                                   # the forms take turns
        for k, f in forms.items():
            ms[k].append(event_ms(f)[1])
    mb = {k: peak_mb(f) for k, f in forms.items()}
    ahead, _, pool = res['pool_ranks']
    s_ahead, s_pool = res['stock']
    flop = 2.0 * n_user * a.news * a.D
    med = {k: statistics.median(v) for k, v in ms.items()}
    L = _lib.lib()
    return {'tool': 'pool_rank_bench', 'users': n_user, 'news': a.news, 'D': a.D, 'E': a.history, 'targets_per_user': per_user, 'K': a.K,
            'rounds': a.rounds,
            'pool_ranks_ms': round(med['pool_ranks'], 3), 'pool_ranks_min_ms': round(min(ms['pool_ranks']), 3),
            'topk_ms': round(med['topk'], 3), 'topk_min_ms': round(min(ms['topk']), 3),
            'stock_ms': round(med['stock'], 3), 'stock_min_ms': round(min(ms['stock']), 3),
            'pool_ranks_over_topk': round(med['pool_ranks'] / med['topk'], 3), 'stock_over_pool_ranks': round(med['stock'] / med['pool_ranks'], 2),
            'pool_ranks_TF': round(flop / (med['pool_ranks'] * 1e-3) / 1e12, 1),
            'pool_ranks_share_of_fp32_matrix_peak': round(flop / (med['pool_ranks'] * 1e-3) / 1e12 / PEAK_TF, 3),
            'pool_ranks_peak_MB': round(mb['pool_ranks'], 2), 'topk_peak_MB': round(mb['topk'], 2), 'stock_peak_MB': round(mb['stock'], 1),
            'pool_ranks_workspace_MB': round(L.nnr_pool_rank_workspace_bytes(n_user, a.news, n_user * per_user) / 2 ** 20, 2),
            'topk_workspace_MB': round(L.nnr_topk_workspace_bytes(n_user, a.news, a.K) / 2 ** 20, 2),
            'ahead_equal_share': round(float((ahead.view(n_user, per_user).long() == s_ahead).float().mean()), 5),
            'max_abs_ahead_diff': int((ahead.view(n_user, per_user).long() - s_ahead).abs().max()),
            'pool_size_equal': bool((pool.long() == s_pool).all()), 'skipped_share': round(float((ahead < 0).float().mean()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', default='50000,64', type=lambda s: [int(x) for x in s.split(',')])
    ap.add_argument('--targets', default='1,8', type=lambda s: [int(x) for x in s.split(',')])
    ap.add_argument('--news', type=int, default=42000)
    ap.add_argument('--D', type=int, default=500)
    ap.add_argument('--history', type=int, default=50)
    ap.add_argument('--K', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pool_rank_bench needs a GPU: a timing taken elsewhere says nothing about this path')
    g = torch.Generator(device='cuda').manual_seed(0)
    reps = torch.randn((a.news, a.D), device='cuda', generator=g)
    valid = torch.ones(a.news, device='cuda', dtype=torch.uint8)
    valid[0] = 0
    for n_user in a.users:
        for per_user in a.targets:
            d = point(n_user, per_user, a, reps, valid, g)
            d.update(device=torch.cuda.get_device_name(0), build=_lib.build_id())
            print(json.dumps(d), flush=True)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
