#!/usr/bin/env python3
"""Listwise evaluation against the cached per-sample form (profiles/list_eval_summary.md): compute_scores(cache=True) and
compute_scores_listwise on one synthetic dev split in one session, by default of MIND-small's dev shape (about 42 k news, 73 k impressions,
2.7 M samples: lists of 1..73 candidates, 37 on average; the impressions draw their behaviour row from 50 k distinct users).

  python tools/list_eval_bench.py [--pairs CNN+ATT,MHSA+MHSA,MHSA+SUE,CNN+CATT] [--impressions 73000] [--news 42000] [--users 50000]
                                  [--max-list 73] [--batch 256] [--candidates-per-row 8]

Per pair: device events around one whole evaluation of each form, after one warm-up evaluation of that form; then the nnr_list_scores launch
alone, on the tables the evaluation built (events around 20 launches, divided by 20) with its read rate (two rows of D floats and two int32
indices per sample).  One JSON line per pair on stdout, with the library's build id."""
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
from nnr_amd.corpus import from_synth_lists                                     # noqa: E402
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
    ap.add_argument('--pairs', default='CNN+ATT,MHSA+MHSA,MHSA+SUE,CNN+CATT')
    ap.add_argument('--impressions', type=int, default=73000)
    ap.add_argument('--news', type=int, default=42000)
    ap.add_argument('--users', type=int, default=50000)
    ap.add_argument('--max-list', type=int, default=73)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--candidates-per-row', type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('list_eval_bench needs a GPU: a timing taken elsewhere says nothing about the evaluation path')
    rng = np.random.default_rng(0)
    sizes = rng.integers(1, a.max_list + 1, size=a.impressions)
    synth = SynthCorpus(SynthSpec(vocabulary_size=VOCAB, news_pool=a.news, seed=3))
    dc = from_synth_lists(synth, sizes, rng, 'cuda', distinct_users=a.users)
    seen = {}
    launch = ops.list_scores

    def capture(user, reps, row, cand, scores=None, check=True):
        seen.update(user=user, reps=reps, row=row, cand=cand)
        return launch(user, reps, row, cand, scores, check)

    for pair in a.pairs.split(','):
        news, user = pair.split('+')
        torch.manual_seed(0)
        model = Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user], corpus_sizes=dict(vocabulary_size=VOCAB)))
        model.initialize()
        model = model.cuda()
        E.compute_scores(model, dc, a.batch, cache=True)
        ref, cached_ms = timed(lambda: E.compute_scores(model, dc, a.batch, cache=True))
        E.compute_scores_listwise(model, dc, sizes, a.batch, candidates_per_row=a.candidates_per_row)
        ops.list_scores = capture
        try:
            got, list_ms = timed(lambda: E.compute_scores_listwise(model, dc, sizes, a.batch, candidates_per_row=a.candidates_per_row))
        finally:
            ops.list_scores = launch
        st = dict(E.LAST_STATS)
        out = torch.empty(dc.num, device='cuda')
        _, k_ms = timed(lambda: [launch(seen['user'], seen['reps'], seen['row'], seen['cand'], out, False) for _ in range(20)])
        k_ms /= 20
        D = seen['reps'].shape[1]
        print(json.dumps({'tool': 'list_eval_bench', 'pair': pair, 'samples': dc.num, 'impressions': a.impressions, 'news_encoded': st['encoder_rows'],
                          'batch': a.batch, 'cached_ms': round(cached_ms, 1), 'listwise_ms': round(list_ms, 1),
                          'speedup': round(cached_ms / list_ms, 2), 'user_rows': st['user_rows'],
                          'user_rows_ratio': round(dc.num / st['user_rows'], 2), 'candidates_per_row': st['candidates_per_row'], 'D': D,
                          'list_scores_us': round(k_ms * 1e3, 1), 'list_scores_read_GBps': round(dc.num * (8.0 * D + 8) / (k_ms * 1e-3) / 1e9, 1),
                          'max_abs_diff': float((got - ref).abs().max()), 'max_abs_score': float(ref.abs().max()),
                          'device': torch.cuda.get_device_name(0), 'build': _lib.build_id()}), flush=True)
        seen.clear()
        del model, ref, got, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
