#!/usr/bin/env python3
"""Measurements of the DSSM baseline and its kernels (profiles/dssm_summary.md).  Seeded synthetic tf-idf term vectors (nnr_amd.synth.
tfidf_rows), the reference's default sizes (user_word_num 3200, news_word_num 200, 1 + 4 candidates, hidden = feature = 512), HIP events
around blocks of `--steps` iterations (no device synchronisation inside a block), the variants of a comparison alternated in one process.

  python tools/dssm_bench.py kernel [--batch 64 8]   nnr_wbag_fwd, nnr_wbag_bwd and nnr_cosine_loss alone: duration, and for the bag the GB/s
                                                     of live table rows read (forward) / of gradient rows read per live occurrence (backward)
  python tools/dssm_bench.py model  [--batch 64 8]   one forward + backward (loss included, no optimizer) against the reference's formulation
                                                     (DSSM_model.py:29-36) in stock torch ops with torch autograd, same inputs and weights
  python tools/dssm_bench.py step   [--batch 64 8]   the full train step: DssmTrainer.train_step against the stock formulation followed by
                                                     clip_grad_norm_ + torch.optim.Adam (DSSM_main.py:62-69)

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from nnr_amd import _lib, ops                                                   # noqa: E402
from nnr_amd.dssm import DSSM, DssmCorpus, DssmTrainer, make_dssm_config        # noqa: E402
from nnr_amd.synth import tfidf_rows                                            # noqa: E402
from npa_bench import alternate                                                 # noqa: E402


def corpus_and_batch(a, B, cfg):
    rng = np.random.default_rng(7)
    U, M = max(4 * B, 64), max(16 * B, 256)
    ui, uw = tfidf_rows(rng, U, cfg.user_word_num, a.vocabulary_size)
    ni, nw = tfidf_rows(rng, M, cfg.news_word_num, a.vocabulary_size)
    ui[0, 0], ni[0, 0] = a.vocabulary_size - 1, a.vocabulary_size - 1           # pins V = max id + 1
    corpus = DssmCorpus(ui, uw, ni, nw, 'cuda')
    us = torch.as_tensor(rng.permutation(U)[:B].astype(np.int32)).cuda()
    ns = torch.as_tensor(rng.integers(0, M, (B, 1 + cfg.negative_sample_num)).astype(np.int32)).cuda()
    return corpus, us, ns


def build(a, B):
    cfg = make_dssm_config(['--batch_size=%d' % B, '--dropout_rate=%g' % a.dropout])
    corpus, us, ns = corpus_and_batch(a, B, cfg)
    cfg.vocabulary_size = corpus.vocabulary_size
    torch.manual_seed(0)
    model = DSSM(cfg)
    model.initialize()
    return cfg, model.cuda().train(), corpus, us, ns


def stock_forward(w, batch, p):
    """DSSM_model.py:29-36 in stock torch ops."""
    ui, uw, _, ni, nw, _ = batch
    d = lambda x: F.dropout(x, p, True)
    ue = d(F.embedding(ui, w['word_embedding.weight']) * uw.unsqueeze(2)).sum(dim=1)
    ne = d(F.embedding(ni, w['word_embedding.weight']) * nw.unsqueeze(3)).sum(dim=2)
    tower = lambda x: d(torch.tanh(F.linear(d(torch.tanh(F.linear(x, w['W3.weight'], w['W3.bias']))), w['W4.weight'], w['W4.bias'])))
    uy, ny = tower(ue).unsqueeze(1), tower(ne)
    logits = (uy * ny).sum(dim=2) / (torch.norm(uy, dim=2) * torch.norm(ny, dim=2))
    return logits, -torch.log_softmax(logits, dim=1).select(1, 0).mean()


def medians(t):
    return {k: float(np.median(v)) for k, v in t.items()}


def mode_kernel(a):
    res = {}
    for B in a.batch:
        cfg, model, corpus, us, ns = build(a, B)
        E, V = cfg.DSSM_hidden_dim, corpus.vocabulary_size
        N = ns.shape[1]
        sa, sb = (corpus.user_ids, corpus.user_w, us), (corpus.news_ids, corpus.news_w, ns.reshape(-1).contiguous())
        table = model.word_embedding.weight.detach()
        dev = dict(device='cuda', dtype=torch.float32)
        out, dout, dtable = torch.empty((B + B * N, E), **dev), torch.randn((B + B * N, E), **dev), torch.zeros_like(table)
        cap = B * cfg.user_word_num + B * N * cfg.news_word_num
        plan = ops.WbagPlan(cap, E, V, torch.device('cuda'))
        ops.wbag_fwd(table, sa, sb, a.dropout, 1, 2, out, plan)
        plan.sort()
        Fd = cfg.DSSM_feature_dim
        y = torch.randn((B + B * N, Fd), **dev)
        logits, loss, dl, dy, ws = torch.empty((B, N), **dev), torch.empty((), **dev), torch.empty((B, N), **dev), torch.empty_like(y), torch.empty(B, **dev)
        torch.cuda.synchronize()
        live = int((corpus.user_w[us.long()] != 0).sum()) + int((corpus.news_w[ns.reshape(-1).long()] != 0).sum())
        words = int(torch.unique(plan.tok[plan.tok >= 0]).numel())
        v = {'wbag_fwd': lambda i: ops.wbag_fwd(table, sa, sb, a.dropout, 1, 2, out, plan),
             'wbag_bwd': lambda i: ops.wbag_bwd(dout, sa, sb, a.dropout, 1, 2, plan, dtable),
             'cosine_loss': lambda i: ops.cosine_loss(y[:B], y[B:], B, N, Fd, logits, loss, dl, dy[:B], dy[B:], ws)}
        t = alternate(v, a.steps, a.warmup, a.rounds)
        ops.join_extra_streams()
        torch.cuda.synchronize()
        med = medians(t)
        res['batch%d' % B] = {'shape': dict(na=B, La=cfg.user_word_num, nb=B * N, Lb=cfg.news_word_num, E=E, V=V, F=Fd), 'ms': t, 'median_ms': med,
                              'live_positions': live, 'live_fraction': round(live / cap, 4), 'distinct_words': words,
                              'live_row_GBps': {'fwd': round(4.0 * E * live / med['wbag_fwd'] / 1e6, 1), 'bwd': round(4.0 * E * live / med['wbag_bwd'] / 1e6, 1)},
                              'gathered_buffer_bytes_avoided': 4.0 * E * cap}
    return res


def _pair(a, B, step):
    cfg, model, corpus, us, ns = build(a, B)
    batch = corpus.gather(us, ns)
    w = {k: v.detach().clone().requires_grad_() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(w.values()), lr=cfg.lr, weight_decay=cfg.weight_decay)
    trainer = DssmTrainer(model, cfg)

    def stock(i):
        _, loss = stock_forward(w, batch, a.dropout)
        opt.zero_grad()
        loss.backward()
        if step:
            torch.nn.utils.clip_grad_norm_(list(w.values()), cfg.gradient_clip_norm)
            opt.step()

    def fused(i):
        if step:
            trainer.train_step((corpus, us, ns))
        else:
            trainer.forward_backward((corpus, us, ns))
    torch.cuda.reset_peak_memory_stats()
    fused(0)
    torch.cuda.synchronize()
    peak_fused = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stock(0)
    torch.cuda.synchronize()
    peak_stock = torch.cuda.max_memory_allocated()
    t = alternate({'nnr_amd': fused, 'stock_torch': stock}, a.steps, a.warmup, a.rounds)
    ops.join_extra_streams()
    torch.cuda.synchronize()
    med = medians(t)
    return {'ms': t, 'median_ms': med, 'speedup_vs_stock': round(med['stock_torch'] / med['nnr_amd'], 3),
            'peak_allocated_MB': {'nnr_amd': round(peak_fused / 2 ** 20, 1), 'stock_torch': round(peak_stock / 2 ** 20, 1)}}


def mode_model(a):
    return {'batch%d' % B: _pair(a, B, step=False) for B in a.batch}


def mode_step(a):
    return {'batch%d' % B: _pair(a, B, step=True) for B in a.batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'model', 'step'])
    ap.add_argument('--batch', type=int, nargs='+', default=[64, 8])
    ap.add_argument('--vocabulary_size', type=int, default=60000)
    ap.add_argument('--dropout', type=float, default=0.0)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    res = {'kernel': mode_kernel, 'model': mode_model, 'step': mode_step}[a.mode](a)
    print(json.dumps({'mode': a.mode, 'dropout': a.dropout, 'steps': a.steps, 'rounds': a.rounds, 'build': _lib.build_id(), 'result': res}))


if __name__ == '__main__':
    main()
