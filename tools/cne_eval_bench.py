#!/usr/bin/env python3
"""De-duplicated evaluation of the rank-pairing CNE encoders against the per-sample form (profiles/cne_eval_summary.md):
compute_scores(cache=False) and compute_scores_dedup on one synthetic dev split in one session, the split of tools/list_eval_bench.py (by
default MIND-small's dev shape: about 42 k news, 73 k impressions, 2.7 M samples; the impressions draw their behaviour row from 50 k users).

  python tools/cne_eval_bench.py [--pairs CNE+SUE,CNE+ATT] [--impressions 73000] [--news 42000] [--users 50000] [--max-list 73]
                                 [--batch 96] [--window 64] [--no-warmup]

Per pair: device events around one whole evaluation of each form, after one warm-up evaluation of that form (--no-warmup: after a warm-up on
the split's first 20 batches only, for sizes at which a second per-sample evaluation costs too much); then the nnr_cne_pair_triples launch
alone, over one window and over the whole split (events around 20 launches, divided by 20).  One JSON line per pair on stdout, with the
library's build id."""
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
from nnr_amd.config import make_config                                          # noqa: E402
from nnr_amd.corpus import DeviceCorpus, from_synth_lists                       # noqa: E402
from nnr_amd.model import Model                                                 # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus                                # noqa: E402

VOCAB = 30000


def timed(fn):
    """(result, milliseconds) of fn() between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return out, start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', default='CNE+SUE,CNE+ATT')
    ap.add_argument('--impressions', type=int, default=73000)
    ap.add_argument('--news', type=int, default=42000)
    ap.add_argument('--users', type=int, default=50000)
    ap.add_argument('--max-list', type=int, default=73)
    ap.add_argument('--batch', type=int, default=96)
    ap.add_argument('--window', type=int, default=64)
    ap.add_argument('--no-warmup', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cne_eval_bench needs a GPU: a timing taken elsewhere says nothing about the evaluation path')
    rng = np.random.default_rng(0)
    sizes = rng.integers(1, a.max_list + 1, size=a.impressions)
    synth = SynthCorpus(SynthSpec(vocabulary_size=VOCAB, news_pool=a.news, seed=3))
    dc = from_synth_lists(synth, sizes, rng, 'cuda', distinct_users=a.users)
    small = None
    if a.no_warmup:                                       # the same tables, the first 20 batches' samples
        k = min(dc.num, 20 * a.batch)
        small = DeviceCorpus(
            dict({key: dc.t[key].cpu().numpy() for key in dc.t if key.startswith('news_')},
                 beh_user=dc.t['beh_user'][:k].cpu().numpy(), beh_history=dc.t['beh_history'][:k].cpu().numpy(),
                 beh_history_mask=dc.t['beh_history_mask'][:k].cpu().numpy()), 'cuda', dc.category_num)
        small.set_samples(dc.samples[:k].cpu().numpy())
    hist, cand = dc.t['beh_history'].contiguous(), dc.samples[:, 0].contiguous()
    tlen, clen = E.news_lengths(dc)
    span = min(dc.num, a.window * a.batch)
    ops.cne_pair_triples(hist, cand, tlen, clen, a.batch)          # (checks the tables once; the first launch loads the code object)
    _, one_ms = timed(lambda: [ops.cne_pair_triples(hist, cand, tlen, clen, a.batch, 0, span, check=False) for _ in range(20)])
    _, all_ms = timed(lambda: [ops.cne_pair_triples(hist, cand, tlen, clen, a.batch, check=False) for _ in range(20)])
    for pair in a.pairs.split(','):
        news, user = pair.split('+')
        torch.manual_seed(0)
        model = Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user], corpus_sizes=dict(vocabulary_size=VOCAB)))
        model.initialize()
        model = model.cuda()
        warm = small if small is not None else dc
        E.compute_scores(model, warm, a.batch, cache=False)
        ref, plain_ms = timed(lambda: E.compute_scores(model, dc, a.batch, cache=False))
        plain = dict(E.LAST_STATS)
        E.compute_scores_dedup(model, warm, a.batch, window=a.window)
        got, dedup_ms = timed(lambda: E.compute_scores_dedup(model, dc, a.batch, window=a.window))
        st = dict(E.LAST_STATS)
        print(json.dumps({'tool': 'cne_eval_bench', 'pair': pair, 'samples': dc.num, 'impressions': a.impressions, 'batch': a.batch,
                          'window': a.window, 'warmup': 'first 20 batches' if a.no_warmup else 'whole split',
                          'per_sample_ms': round(plain_ms, 1), 'dedup_ms': round(dedup_ms, 1), 'speedup': round(plain_ms / dedup_ms, 2),
                          'per_sample_rows': st['per_sample_rows'], 'rows_after_pad_dedup': plain['encoder_rows'], 'triples': st['triples'],
                          'triples_per_row': round(st['triples'] / st['per_sample_rows'], 4), 'distinct_news': st['distinct_news'],
                          'windows': st['windows'], 'plan_one_window_us': round(one_ms / 20 * 1e3, 1), 'plan_whole_split_us': round(all_ms / 20 * 1e3, 1),
                          'max_abs_diff': float((got - ref).abs().max()), 'max_abs_score': float(ref.abs().max()),
                          'device': torch.cuda.get_device_name(0), 'build': _lib.build_id()}), flush=True)
        del model, ref, got
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
