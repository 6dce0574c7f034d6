#!/usr/bin/env python3
"""Top-K recommendation (profiles/recommend_summary.md): the fused score-and-select launch (nnr_topk_scores) and evaluate.recommend against
stock torch on the same device in the same session.

  python tools/recommend_bench.py [--legs kernel,e2e] [--users 50000,64] [--news 42000] [--D 500] [--K 10] [--history 50]
                                  [--pair CNN+ATT] [--impressions 73000] [--distinct-users 50000] [--batch 256] [--reps 5]

The baseline is what a user of stock ops has to write: the user rows in chunks sized so that a chunk's [chunk, news] float32 scores are one
1 GB block; per chunk `user[c] @ reps.T`, a masked_fill for the pool, an index-put of -inf for the history lists (a scatter_reduce, which needs no host
sync), torch.topk.

kernel: random normal tables, a pool of every row but row 0, `--history` random excluded rows per user (a fifth of the slots are -1 pads);
        one point per entry of --users.  Events around --reps launches after one warm-up, divided; TF = 2 * users * news * D / time against
        the 157.3 TF fp32 matrix peak; peak memory = torch's peak allocated bytes above the inputs during one call.
e2e:    a synthetic MIND-small dev split (tools/list_eval_bench.py's), recommend() for the first row of every impression and for the first
        64 of them; the launch alone and the baseline on the tables that evaluation built.
One JSON line per point on stdout, with the library's build id."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops                                                   # noqa: E402
from nnr_amd import evaluate as E                                               # noqa: E402

VOCAB = 30000
PEAK_TF = 157.3


def timed(fn, reps=1):
    """(result of the last call, milliseconds per call) of `reps` calls of fn() between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return out, start.elapsed_time(end) / reps


def peak_mb(fn):
    """(result, MB that torch's allocator peaked at above what was allocated before the call)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def stock_topk(user, reps, K, valid, exclude, block_bytes=1 << 30):
    """The chunked stock-torch form: (idx int64 [n_user, K], score [n_user, K]); ineligible picks come back as -inf scores."""
    n_user, n_reps = user.shape[0], reps.shape[0]
    chunk = max(1, block_bytes // (4 * n_reps))
    out_ = ~valid.bool() if valid is not None else None
    idx = torch.empty((n_user, K), device=user.device, dtype=torch.int64)
    score = torch.empty((n_user, K), device=user.device, dtype=torch.float32)
    for s in range(0, n_user, chunk):
        sc = user[s:s + chunk] @ reps.t()
        if out_ is not None:
            sc.masked_fill_(out_, float('-inf'))
        if exclude is not None:
            ex = exclude[s:s + chunk].long()
            live = (ex >= 0) & (ex < n_reps)
            # no host sync: a dead entry takes the minimum with +inf at column 0, which changes nothing; a live one with -inf
            sc.scatter_reduce_(1, torch.where(live, ex, 0), torch.where(live, float('-inf'), float('inf')).to(sc.dtype), 'amin')
        score[s:s + chunk], idx[s:s + chunk] = torch.topk(sc, K, dim=1)
    return idx, score


def compare(tag, user, reps, K, valid, exclude, reps_n):
    """One JSON-ready dict: the fused launch and the stock form on the same tables."""
    n_user, D = user.shape
    n_reps = reps.shape[0]
    fused = lambda: ops.topk_scores(user, reps, K, valid=valid, exclude=exclude, check=False)
    stock = lambda: stock_topk(user, reps, K, valid, exclude)
    fused()
    stock()
    (fi, fs), f_ms = timed(fused, reps_n)
    (si, ss), s_ms = timed(stock, max(1, reps_n // 2))
    _, f_mb = peak_mb(fused)
    _, s_mb = peak_mb(stock)
    same = float((fi.long() == torch.where(torch.isneginf(ss), -1, si)).float().mean())
    flop = 2.0 * n_user * n_reps * D
    return {'tool': 'recommend_bench', 'leg': tag, 'users': n_user, 'news': n_reps, 'D': D, 'K': K,
            'E': 0 if exclude is None else exclude.shape[1], 'fused_ms': round(f_ms, 3), 'fused_TF': round(flop / (f_ms * 1e-3) / 1e12, 1),
            'fused_share_of_fp32_matrix_peak': round(flop / (f_ms * 1e-3) / 1e12 / PEAK_TF, 3), 'stock_ms': round(s_ms, 3),
            'stock_over_fused': round(s_ms / f_ms, 2), 'fused_peak_MB': round(f_mb, 1), 'stock_peak_MB': round(s_mb, 1),
            'workspace_MB': round(_lib.lib().nnr_topk_workspace_bytes(n_user, n_reps, K) / 2 ** 20, 2),
            'picks_equal_share': round(same, 5), 'max_abs_score_diff': float((fs - ss).abs().nan_to_num(0.0).max())}


def leg_kernel(a):
    g = torch.Generator(device='cuda').manual_seed(0)
    reps = torch.randn((a.news, a.D), device='cuda', generator=g)
    valid = torch.ones(a.news, device='cuda', dtype=torch.uint8)
    valid[0] = 0
    for n_user in a.users:
        user = torch.randn((n_user, a.D), device='cuda', generator=g)
        ex = torch.randint(1, a.news, (n_user, a.history), device='cuda', generator=g, dtype=torch.int32)
        ex[torch.rand((n_user, a.history), device='cuda', generator=g) < 0.2] = -1
        emit(compare('kernel', user, reps, a.K, valid, ex, a.reps))
        del user, ex
        torch.cuda.empty_cache()


def leg_e2e(a):
    from nnr_amd.config import make_config
    from nnr_amd.corpus import from_synth_lists
    from nnr_amd.model import Model
    from nnr_amd.synth import SynthSpec, SynthCorpus
    rng = np.random.default_rng(0)
    sizes = rng.integers(1, 74, size=a.impressions)
    dc = from_synth_lists(SynthCorpus(SynthSpec(vocabulary_size=VOCAB, news_pool=a.news, seed=3)), sizes, rng, 'cuda',
                          distinct_users=a.distinct_users)
    first = np.zeros(a.impressions, dtype=np.int64)
    np.cumsum(sizes[:-1], out=first[1:])
    news, user = a.pair.split('+')
    torch.manual_seed(0)
    model = Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user], corpus_sizes=dict(vocabulary_size=VOCAB)))
    model.initialize()
    model = model.cuda()
    seen = {}
    launch = ops.topk_scores

    def capture(user, reps, K, valid=None, exclude=None, check=True):
        seen.update(user=user, reps=reps, valid=valid, exclude=exclude)
        return launch(user, reps, K, valid, exclude, check)

    for rows in (first, first[:64]):
        E.recommend(model, dc, a.K, rows=rows, batch_size=a.batch)
        ops.topk_scores = capture
        try:
            _, ms = timed(lambda: E.recommend(model, dc, a.K, rows=rows, batch_size=a.batch))
            _, mb = peak_mb(lambda: E.recommend(model, dc, a.K, rows=rows, batch_size=a.batch))
        finally:
            ops.topk_scores = launch
        st = dict(E.LAST_STATS)
        out = compare('e2e', seen['user'], seen['reps'], a.K, seen['valid'], seen['exclude'], a.reps)
        out.update(pair=a.pair, rows=st['rows'], user_rows=st['user_rows'], encoder_rows=st['encoder_rows'], pool=st['pool'],
                   recommend_ms=round(ms, 1), recommend_peak_MB=round(mb, 1))
        emit(out)
        seen.clear()
        torch.cuda.empty_cache()


def emit(d):
    d.update(device=torch.cuda.get_device_name(0), build=_lib.build_id())
    print(json.dumps(d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='kernel,e2e')
    ap.add_argument('--users', default='50000,64', type=lambda s: [int(x) for x in s.split(',')])
    ap.add_argument('--news', type=int, default=42000)
    ap.add_argument('--D', type=int, default=500)
    ap.add_argument('--K', type=int, default=10)
    ap.add_argument('--history', type=int, default=50)
    ap.add_argument('--pair', default='CNN+ATT')
    ap.add_argument('--impressions', type=int, default=73000)
    ap.add_argument('--distinct-users', type=int, default=50000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('recommend_bench needs a GPU: a timing taken elsewhere says nothing about this path')
    for leg in a.legs.split(','):
        {'kernel': leg_kernel, 'e2e': leg_e2e}[leg](a)


if __name__ == '__main__':
    main()
