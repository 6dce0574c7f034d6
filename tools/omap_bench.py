#!/usr/bin/env python3
"""Measurements of the OMAP user encoder (profiles/omap_summary.md).  Seeded synthetic data, MIND-200k shapes, HIP events around blocks of
`--steps` iterations (no device synchronisation inside a block), the variants of a comparison alternated in one process.

  python tools/omap_bench.py kernel  [--batch 64 8]   the reference's formulation of OMAP (userEncoders.py:357-369: bmm, masked softmax, residual,
                                                      matmul, softmax over the heads, three more bmm) in stock torch ops with torch's autograd
                                                      vs OMAP.encode_user, forward + backward, same inputs / weights
  python tools/omap_bench.py step    [--batch 64]     training step, dropout on: CNE+OMAP vs CNE+CATT vs CNE+ATT, all on the autograd path
  NNR_ONE_STREAM=1 rocprofv3 --kernel-trace --stats -- python tools/omap_bench.py trace
                                                      a few CNE+SUE, CNE+CATT and CNE+OMAP steps on one stream: solo durations of omap_* next to
                                                      cand_attn_* and sue_intra_* at the same B, N, H, D

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib                                      # noqa: E402
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


def build(ne, ue, batch, V):
    cfg = make_config(['--news_encoder=' + ne, '--user_encoder=' + ue, '--dataset=200k', '--batch_size=%d' % batch], corpus_sizes=dict(vocabulary_size=V))
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table)
    model.initialize()
    return cfg, model.cuda().train()


def reference_formulation(hist, cand, mask, W):
    """userEncoders.py:357-369 in stock torch ops with torch's autograd."""
    H, K = hist.shape[1], W.shape[1]
    s = hist.shape[2] ** 0.5
    a = torch.bmm(hist, hist.permute(0, 2, 1)) / s
    alpha = torch.softmax(a.masked_fill(mask.unsqueeze(1).expand(-1, H, -1) == 0, -1e9), dim=2)
    y = hist + torch.bmm(alpha, hist)
    b = torch.matmul(y, W) / s
    beta = torch.softmax(b.masked_fill(mask.unsqueeze(2).expand(-1, -1, K) == 0, -1e9), dim=2)
    archives = torch.bmm(beta.permute(0, 2, 1), y)
    gamma = torch.softmax(torch.bmm(cand, archives.permute(0, 2, 1)) / s, dim=2)
    return torch.bmm(gamma, archives)


def mode_kernel(a):
    res = {}
    for B in a.batch:
        cfg, model = build('CNE', 'OMAP', B, 2000)
        ue = model.user_encoder.eval()                   # (the encoder alone: the regulariser belongs to the step, see mode_step)
        D, H, N = model.news_embedding_dim, cfg.max_history_num, cfg.negative_sample_num + 1
        g = torch.Generator(device='cuda').manual_seed(B)
        hist = (0.3 * torch.randn(B, H, D, device='cuda', generator=g)).requires_grad_()
        cand = (0.3 * torch.randn(B, N, D, device='cuda', generator=g)).requires_grad_()
        dout = torch.randn(B, N, D, device='cuda', generator=g)
        lens = torch.randint(0, H + 1, (B,), device='cuda', generator=g)
        mask = torch.arange(H, device='cuda').unsqueeze(0) < lens.unsqueeze(1)
        ref_w = ue.W.detach().clone().requires_grad_()

        def baseline(i):
            reference_formulation(hist, cand, mask, ref_w).backward(dout)

        def candidate(i):
            ue.encode_user(hist, mask, None, None, None, cand).backward(dout)
        with torch.no_grad():
            err = float((reference_formulation(hist, cand, mask, ref_w) - ue.encode_user(hist, mask, None, None, None, cand)).abs().max())
        t = alternate({'torch_reference_formulation': baseline, 'omap_encode_user': candidate}, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['batch%d' % B] = {'ms_fwd_bwd': t, 'median_ms': med, 'speedup': round(med['torch_reference_formulation'] / med['omap_encode_user'], 2),
                              'max_abs_diff_of_outputs': err, 'shape': dict(B=B, N=N, H=H, K=cfg.OMAP_head_num, D=D)}
    return res


def _step_fn(trainer, batches):
    return lambda i: trainer.train_step(batches[i % len(batches)])


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(8)]
    variants, paths = {}, {}
    trainers = {}
    for ue in ('OMAP', 'CATT', 'ATT'):
        cfg, model = build('CNE', ue, B, a.vocabulary_size)
        trainers[ue] = Trainer(model, cfg)
        variants['CNE+' + ue] = _step_fn(trainers[ue], batches)
    t = alternate(variants, a.steps, a.warmup, a.rounds)
    for ue, tr in trainers.items():
        paths['CNE+' + ue] = tr.last_path
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {'batch': B, 'dropout_rate': 0.2, 'ms_per_step': t, 'median_ms': med, 'path': paths,
            'omap_minus_att_ms': round(med['CNE+OMAP'] - med['CNE+ATT'], 4), 'catt_minus_att_ms': round(med['CNE+CATT'] - med['CNE+ATT'], 4)}


def mode_trace(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(2)]
    out = {}
    for ue in ('SUE', 'CATT', 'OMAP'):
        cfg, model = build('CNE', ue, B, a.vocabulary_size)
        tr = Trainer(model, cfg, replay=False)
        for i in range(a.trace_steps):
            tr.train_step(batches[i % 2])
        torch.cuda.synchronize()
        out['CNE+' + ue] = tr.last_path
    return {'batch': B, 'steps_each': a.trace_steps, 'path': out, 'one_stream': os.environ.get('NNR_ONE_STREAM') == '1'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'step', 'trace'])
    ap.add_argument('--batch', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trace_steps', type=int, default=6)
    ap.add_argument('--vocabulary_size', type=int, default=60000)
    a = ap.parse_args()
    if a.batch is None:
        a.batch = [64, 8] if a.mode == 'kernel' else [64]
    _lib.lib()
    res = {'kernel': mode_kernel, 'step': mode_step, 'trace': mode_trace}[a.mode](a)
    print(json.dumps({'mode': a.mode, 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(0), 'steps_per_block': a.steps,
                      'rounds': a.rounds, 'result': res}))


if __name__ == '__main__':
    main()
