#!/usr/bin/env python3
"""The archive form of recommend / rank_in_pool (profiles/archive_rank_summary.md): nnr_topk_archive_scores and nnr_pool_archive_ranks
against this build's plain launches and against stock torch, on the same device in the same session, in turns.

  python tools/archive_rank_bench.py [--legs kernel,e2e] [--users 50000,64] [--news 42000] [--D 500] [--K 10] [--history 50] [--archives 3]
                                     [--pair CNN+OMAP] [--impressions 73000] [--distinct-users 50000] [--batch 256] [--reps 3]

kernel: random normal tables, a pool of every row but row 0, `--history` random excluded rows per user (a fifth of the slots are -1 pads), one
        clicked target per user; one point per entry of --users.  The archive launch does A times the plain launch's matrix work plus the
        combine, so every point carries the plain launch on one of the A archives, A times that, and the ratio.  The stock form is what a
        user of stock ops has to write: the [U * A, D] table in chunks sized so that a chunk's [chunk * A, news] float32 products are one
        1 GB block; per chunk a matmul, a softmax over the archives of scale * products, the weighted sum, a masked_fill for the pool, an
        index-put of -inf for the history lists, then torch.topk -- or, for the ranks, a compare with the target's score and a sum.
e2e:    a synthetic MIND-small dev split (tools/list_eval_bench.py's), recommend() for the first row of every impression and for 64 of them.
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
from tools.recommend_bench import VOCAB, PEAK_TF, timed, peak_mb                # noqa: E402


def stock_scores(user3, reps, scale, valid, exclude, s, chunk):
    """[chunk, news] combined scores of users s .. s + chunk - 1, -inf over the ineligible positions."""
    u = user3[s:s + chunk]
    c, A, D = u.shape
    p = (u.reshape(c * A, D) @ reps.t()).view(c, A, -1)
    sc = (torch.softmax(p * scale, dim=1) * p).sum(dim=1)
    if valid is not None:
        sc.masked_fill_(~valid.bool(), float('-inf'))
    if exclude is not None:
        ex = exclude[s:s + chunk].long()
        live = (ex >= 0) & (ex < reps.shape[0])
        sc.scatter_reduce_(1, torch.where(live, ex, 0), torch.where(live, float('-inf'), float('inf')).to(sc.dtype), 'amin')
    return sc


def stock_topk(user3, reps, scale, K, valid, exclude, block_bytes=1 << 30):
    n_user, A = user3.shape[:2]
    chunk = max(1, block_bytes // (4 * reps.shape[0] * A))
    idx = torch.empty((n_user, K), device=reps.device, dtype=torch.int64)
    score = torch.empty((n_user, K), device=reps.device, dtype=torch.float32)
    for s in range(0, n_user, chunk):
        score[s:s + chunk], idx[s:s + chunk] = torch.topk(stock_scores(user3, reps, scale, valid, exclude, s, chunk), K, dim=1)
    return idx, score


def stock_ranks(user3, reps, scale, target, valid, exclude, block_bytes=1 << 30):
    """ahead int64 [n_user] for ONE target per user (ties by row; -1 for an ineligible target)."""
    n_user, A = user3.shape[:2]
    chunk = max(1, block_bytes // (4 * reps.shape[0] * A))
    ahead = torch.empty(n_user, device=reps.device, dtype=torch.int64)
    rows = torch.arange(reps.shape[0], device=reps.device)
    for s in range(0, n_user, chunk):
        sc = stock_scores(user3, reps, scale, valid, exclude, s, chunk)
        tg = target[s:s + chunk].long()
        ts = sc.gather(1, tg.view(-1, 1))
        before = ((sc > ts) | ((sc == ts) & (rows.view(1, -1) < tg.view(-1, 1)))).sum(dim=1)
        ahead[s:s + chunk] = torch.where(torch.isneginf(ts.view(-1)), -1, before)
    return ahead


def leg_kernel(a):
    g = torch.Generator(device='cuda').manual_seed(0)
    A, scale = a.archives, 1.0 / float(np.sqrt(a.D))
    reps = torch.randn((a.news, a.D), device='cuda', generator=g)
    valid = torch.ones(a.news, device='cuda', dtype=torch.uint8)
    valid[0] = 0
    for n_user in a.users:
        user3 = torch.randn((n_user, A, a.D), device='cuda', generator=g)
        one = user3[:, 0].contiguous()
        ex = torch.randint(1, a.news, (n_user, a.history), device='cuda', generator=g, dtype=torch.int32)
        ex[torch.rand((n_user, a.history), device='cuda', generator=g) < 0.2] = -1
        t_off = torch.arange(n_user + 1, device='cuda', dtype=torch.int32)
        t_news = torch.randint(1, a.news, (n_user,), device='cuda', generator=g, dtype=torch.int32)
        legs = {
            'topk_archive': lambda: ops.topk_scores(user3, reps, a.K, valid=valid, exclude=ex, check=False, archives=A, scale=scale),
            'topk_plain': lambda: ops.topk_scores(one, reps, a.K, valid=valid, exclude=ex, check=False),
            'topk_stock': lambda: stock_topk(user3, reps, scale, a.K, valid, ex),
            'rank_archive': lambda: ops.pool_ranks(user3, reps, t_off, t_news, valid=valid, exclude=ex, check=False, archives=A, scale=scale),
            'rank_plain': lambda: ops.pool_ranks(one, reps, t_off, t_news, valid=valid, exclude=ex, check=False),
            'rank_stock': lambda: stock_ranks(user3, reps, scale, t_news, valid, ex),
        }
        ms, out = {k: [] for k in legs}, {}
        for fn in legs.values():
            fn()                                                                # warm-up
        for _ in range(a.turns):                                                # in turns: every leg sees the same drift of the session
            for k, fn in legs.items():
                out[k], t = timed(fn, a.reps if 'stock' not in k else 1)
                ms[k].append(t)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        _, arch_mb = peak_mb(legs['topk_archive'])
        _, stock_mb = peak_mb(legs['topk_stock'])
        (fi, fs), (si, ss) = out['topk_archive'], out['topk_stock']
        flop = 2.0 * n_user * a.news * a.D * A
        d = {'tool': 'archive_rank_bench', 'leg': 'kernel', 'users': n_user, 'news': a.news, 'D': a.D, 'K': a.K, 'E': a.history, 'archives': A,
             'turns': a.turns, 'picks_equal_share': round(float((fi.long() == torch.where(torch.isneginf(ss), -1, si)).float().mean()), 5),
             'max_abs_score_diff': float((fs - ss).abs().nan_to_num(0.0).max()),
             'ranks_equal_share': round(float((out['rank_archive'][0].long() == out['rank_stock']).float().mean()), 5),
             'topk_archive_TF': round(flop / (med['topk_archive'] * 1e-3) / 1e12, 1),
             'topk_archive_share_of_fp32_matrix_peak': round(flop / (med['topk_archive'] * 1e-3) / 1e12 / PEAK_TF, 3),
             'topk_archive_over_A_plain': round(med['topk_archive'] / (A * med['topk_plain']), 3),
             'rank_archive_over_A_plain': round(med['rank_archive'] / (A * med['rank_plain']), 3),
             'topk_stock_over_archive': round(med['topk_stock'] / med['topk_archive'], 2),
             'rank_stock_over_archive': round(med['rank_stock'] / med['rank_archive'], 2),
             'topk_archive_peak_MB': round(arch_mb, 1), 'topk_stock_peak_MB': round(stock_mb, 1)}
        d.update({k + '_ms': round(v, 3) for k, v in med.items()})
        d.update({k + '_ms_min_max': [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()})
        emit(d)
        del user3, one, ex, out
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
    for rows in (first, first[:64]):
        E.recommend(model, dc, a.K, rows=rows, batch_size=a.batch, archives=True)
        _, ms = timed(lambda: E.recommend(model, dc, a.K, rows=rows, batch_size=a.batch, archives=True))
        _, mb = peak_mb(lambda: E.recommend(model, dc, a.K, rows=rows, batch_size=a.batch, archives=True))
        st = dict(E.LAST_STATS)
        emit({'tool': 'archive_rank_bench', 'leg': 'e2e', 'pair': a.pair, 'rows': st['rows'], 'user_rows': st['user_rows'],
              'encoder_rows': st['encoder_rows'], 'pool': st['pool'], 'K': st['K'], 'archives': st['archives'], 'recommend_ms': round(ms, 1),
              'recommend_peak_MB': round(mb, 1)})
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
    ap.add_argument('--archives', type=int, default=3)
    ap.add_argument('--pair', default='CNN+OMAP')
    ap.add_argument('--impressions', type=int, default=73000)
    ap.add_argument('--distinct-users', type=int, default=50000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--turns', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('archive_rank_bench needs a GPU: a timing taken elsewhere says nothing about this path')
    for leg in a.legs.split(','):
        {'kernel': leg_kernel, 'e2e': leg_e2e}[leg](a)


if __name__ == '__main__':
    main()
