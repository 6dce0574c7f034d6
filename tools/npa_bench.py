#!/usr/bin/env python3
"""Measurements of NPA: the PNE news encoder, the PUE user encoder and the per-title personalised attention kernel (profiles/npa_summary.md).
Seeded synthetic data, MIND-200k shapes, HIP events around blocks of `--steps` iterations (no device synchronisation inside a block), the
variants of a comparison alternated in one process.

  python tools/npa_bench.py kernel  [--batch 64 8]   pers_attn forward and backward vs the cand_attn kernels on the same problem (B' = n, N = 1, the
                                                     query projection expanded to n rows): n = batch * 55 titles, L 32, A 200, F 400, MIND-shaped
                                                     title masks (and an all-live mask for the traffic bound)
  python tools/npa_bench.py encoder [--batch 64 8]   PNE's pooling stage and PUE, forward + backward, vs the reference's formulation of
                                                     CandidateAttention in stock torch ops on the same inputs / weights
  python tools/npa_bench.py step    [--batch 64]     training step, dropout on: CNN+ATT, PNE+ATT and PNE+PUE (all on the autograd path)

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops                                  # noqa: E402
from nnr_amd.config import make_config                        # noqa: E402
from nnr_amd.model import Model                               # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch    # noqa: E402
from nnr_amd.trainer import Trainer                           # noqa: E402


def timed(fn, steps):
    """ms per iteration of `steps` back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternate(variants, steps, warmup, rounds):
    """{name: [ms per iteration, one per round]} with the variants alternated round by round."""
    for fn in variants.values():
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(round(timed(fn, steps), 4))
    return out


def build(ne, ue, batch, V, users=64):
    cfg = make_config(['--news_encoder=' + ne, '--user_encoder=' + ue, '--dataset=200k', '--batch_size=%d' % batch],
                      corpus_sizes=dict(vocabulary_size=V, user_num=users))
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table)
    model.initialize()
    return cfg, model.cuda().train()


def title_masks(B, V):
    """The title masks of one synthetic MIND-shaped batch, candidate titles then history titles: [B * 55, 32] bool."""
    b = to_torch(SynthCorpus(SynthSpec(vocabulary_size=V)).batch(B, np.random.default_rng(100)), 'cuda')
    Lx = b[15].shape[-1]
    return torch.cat([b[16].reshape(-1, Lx), b[4].reshape(-1, Lx)]).bool().contiguous()


def mode_kernel(a):
    res = {}
    Lx, A, F = 32, 200, 400
    for B in a.batch:
        mind = title_masks(B, a.vocabulary_size)
        n, U = mind.shape[0], B
        g = torch.Generator(device='cuda').manual_seed(B)
        dev = dict(device='cuda', dtype=torch.float32)
        Qf, P = torch.randn(n * Lx, A, generator=g, **dev), torch.randn(U, A, generator=g, **dev)
        w2 = torch.randn(A, generator=g, **dev) / A ** 0.5
        feat, dout = torch.randn(n, Lx, F, generator=g, **dev), torch.randn(n, F, generator=g, **dev)
        uidx = (torch.arange(n, device='cuda') % U).to(torch.int32)
        Pn = P[uidx.long()].contiguous()                                  # what the candidate-attention kernels carry: one query row per title
        alpha, out = torch.empty((n, Lx), **dev), torch.empty((n, F), **dev)
        alpha_c, out_c = torch.empty((n, 1, Lx), **dev), torch.empty((n, 1, F), **dev)
        dP, dPn, dQ, dQ_c = torch.empty((U, A), **dev), torch.empty((n, A), **dev), torch.empty((n * Lx, A), **dev), torch.empty((n * Lx, A), **dev)
        dx, dx_c, dw2 = torch.empty((n, Lx, F), **dev), torch.empty((n, Lx, F), **dev), torch.zeros(A, **dev)
        per = {}
        for tag, mask in (('mind_mask', mind), ('all_live', torch.ones_like(mind))):
            v = {
                'pers_attn_fwd': lambda i, m=mask: ops.pers_attn_fwd(Qf, P, uidx, w2, feat, m, n, Lx, A, F, alpha, out),
                'cand_attn_fwd': lambda i, m=mask: ops.cand_attn_fwd(Pn, Qf, w2, feat, m, n, 1, Lx, A, F, ops.ACT_TANH, alpha_c, out_c),
                'pers_attn_bwd': lambda i, m=mask: ops.pers_attn_bwd(Qf, P, uidx, w2, feat, m, alpha, dout, n, Lx, A, F, dP, dQ, dx, dw2),
                'cand_attn_bwd': lambda i, m=mask: ops.cand_attn_bwd(Pn, Qf, w2, feat, m, alpha_c, dout, n, 1, Lx, A, F, ops.ACT_TANH, dPn, dQ_c, dx_c, dw2),
            }
            t = alternate(v, a.steps, a.warmup, a.rounds)
            torch.cuda.synchronize()
            med = {k: float(np.median(x)) for k, x in t.items()}
            diff = dict(out=float((out - out_c.view(n, F)).abs().max()), dfeat=float((dx - dx_c).abs().max()), dQf=float((dQ - dQ_c).abs().max()))
            live = float(mask.float().mean())
            # bytes the algorithm needs with this mask: the Qf rows and feature rows of the live positions once per direction (+ their gradients, written
            # for every position), weights, outputs
            fwd_bytes = 4.0 * n * (live * Lx * (A + F) + Lx + F) + n * Lx
            bwd_bytes = 4.0 * n * (live * Lx * (A + F) + Lx * (A + F) + Lx + F + 4 * A) + n * Lx
            per[tag] = {'ms': t, 'median_ms': med, 'live_fraction': round(live, 4),
                        'speedup_fwd': round(med['cand_attn_fwd'] / med['pers_attn_fwd'], 2),
                        'speedup_bwd': round(med['cand_attn_bwd'] / med['pers_attn_bwd'], 2),
                        'pers_attn_GBps': {'fwd': round(fwd_bytes / med['pers_attn_fwd'] / 1e6, 1), 'bwd': round(bwd_bytes / med['pers_attn_bwd'] / 1e6, 1)},
                        'max_abs_diff_between_the_two': diff}
        res['batch%d' % B] = {'shape': dict(n=n, L=Lx, A=A, F=F, U=U), **per}
    return res


def reference_attention(feature, query, mask, wf, wq, bq, w2):
    """layers.py:225-232 in stock torch ops (query already one row per feature set)."""
    a = torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(feature, wf) + torch.nn.functional.linear(query, wq, bq).unsqueeze(1)), w2).squeeze(2)
    alpha = torch.softmax(a.masked_fill(mask == 0, -1e9), dim=1)
    return torch.bmm(alpha.unsqueeze(1), feature).squeeze(1)


def mode_encoder(a):
    from nnr_amd.layers import personalized_attention
    res = {}
    for B in a.batch:
        cfg, model = build('PNE', 'PUE', B, 2000, users=max(B, 2))
        ne, ue = model.news_encoder, model.user_encoder
        mind = title_masks(B, a.vocabulary_size)
        n, Lx, C, D, H = mind.shape[0], cfg.max_title_length, cfg.cnn_kernel_num, model.news_embedding_dim, cfg.max_history_num
        g = torch.Generator(device='cuda').manual_seed(B)
        c = torch.randn(n, Lx, C, device='cuda', generator=g).requires_grad_()
        rows = (0.1 * torch.randn(B, cfg.user_embedding_dim, device='cuda', generator=g)).requires_grad_()
        dout = torch.randn(n, C, device='cuda', generator=g)
        hist = torch.randn(B, H, D, device='cuda', generator=g).requires_grad_()
        cand = torch.randn(B, 5, D, device='cuda', generator=g)
        dusr = torch.randn(B, 5, D, device='cuda', generator=g)
        lens = torch.randint(0, H + 1, (B,), device='cuda', generator=g)
        hmask = torch.arange(H, device='cuda').unsqueeze(0) < lens.unsqueeze(1)
        uidx = (torch.arange(n, device='cuda') % B).to(torch.int32)

        def weights(mod):
            pa = mod.personalizedAttention
            return [p.detach().clone().requires_grad_() for p in (mod.dense.weight, mod.dense.bias, pa.feature_affine.weight, pa.query_affine.weight,
                                                                   pa.query_affine.bias, pa.attention_affine.weight)]
        wn, wu = weights(ne), weights(ue)

        def pne_ref(i=0):
            q = torch.relu(torch.nn.functional.linear(rows, wn[0], wn[1])).repeat([n // B, 1])
            return reference_attention(c, q, mind, *wn[2:])

        def pne_hip(i=0):
            from nnr_amd import functional as Fn
            q = Fn.LinearFn.apply(rows, ne.dense.weight, ne.dense.bias, ops.ACT_RELU, 0.0, 0)
            return personalized_attention(ne.personalizedAttention, c, q, uidx, mind)

        def pue_ref(i=0):
            q = torch.relu(torch.nn.functional.linear(rows, wu[0], wu[1]))
            return reference_attention(hist, q, hmask, *wu[2:]).unsqueeze(1).expand(-1, 5, -1)

        def pue_hip(i=0):
            return ue.encode_user(hist, hmask, None, None, None, cand, rows)
        with torch.no_grad():
            err = dict(pne=float((pne_ref() - pne_hip()).abs().max()), pue=float((pue_ref() - pue_hip()).abs().max()))
        t = alternate({'pne_torch_reference_formulation': lambda i: pne_ref().backward(dout), 'pne_pooling_stage': lambda i: pne_hip().backward(dout),
                       'pue_torch_reference_formulation': lambda i: pue_ref().backward(dusr), 'pue_encode_user': lambda i: pue_hip().backward(dusr)},
                      a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['batch%d' % B] = {'ms_fwd_bwd': t, 'median_ms': med, 'max_abs_diff_of_outputs': err,
                              'speedup_pne': round(med['pne_torch_reference_formulation'] / med['pne_pooling_stage'], 2),
                              'speedup_pue': round(med['pue_torch_reference_formulation'] / med['pue_encode_user'], 2),
                              'shape': dict(n=n, L=Lx, C=C, B=B, H=H, D=D, A=cfg.attention_dim)}
    return res


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(8)]
    variants, paths, trainers = {}, {}, {}
    for ne, ue in (('CNN', 'ATT'), ('PNE', 'ATT'), ('PNE', 'PUE')):
        cfg, model = build(ne, ue, B, a.vocabulary_size, users=max(B, 2))
        trainers[ne + '+' + ue] = Trainer(model, cfg)
        variants[ne + '+' + ue] = lambda i, tr=trainers[ne + '+' + ue]: tr.train_step(batches[i % len(batches)])
    t = alternate(variants, a.steps, a.warmup, a.rounds)
    for k, tr in trainers.items():
        paths[k] = tr.last_path
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {'batch': B, 'dropout_rate': 0.2, 'ms_per_step': t, 'median_ms': med, 'path': paths}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'encoder', 'step'])
    ap.add_argument('--batch', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--vocabulary_size', type=int, default=60000)
    a = ap.parse_args()
    if a.batch is None:
        a.batch = [64] if a.mode == 'step' else [64, 8]
    _lib.lib()
    res = {'kernel': mode_kernel, 'encoder': mode_encoder, 'step': mode_step}[a.mode](a)
    print(json.dumps({'mode': a.mode, 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(0), 'steps_per_block': a.steps,
                      'rounds': a.rounds, 'result': res}))


if __name__ == '__main__':
    main()
