#!/usr/bin/env python3
"""Measurements of the KCNN news encoder (DKN) and of the kernels of csrc/kcnn.hip (profiles/kcnn_summary.md).  Seeded synthetic data,
MIND-200k shapes (title 32 slots, batch * 55 titles per step, E 300, C 400, window 3, knowledge rows of 100), entity ids written into the
batches here (nnr_amd.synth leaves them zero): a non-zero id on about a fifth of the positions.  HIP events around blocks of `--steps`
iterations (no device synchronisation inside a block), the variants of a comparison alternated in one process.

  python tools/kcnn_bench.py kernel  [--batch 64 8]   the five kernels alone: duration and achieved share of the HBM bandwidth (bytes = every
                                                      operand read once, every result written once)
  python tools/kcnn_bench.py encoder [--batch 64 8]   one encoder call over the batch's batch * 55 titles, forward + backward, dropout on, vs the
                                                      reference's formulation in stock torch ops (F.conv2d = MIOpen) with torch autograd on the
                                                      same inputs / weights
  python tools/kcnn_bench.py step    [--batch 64]     training step of KCNN+CATT (autograd path), dropout on, next to CNN+CATT

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

from nnr_amd import _lib, ops                                  # noqa: E402
from nnr_amd import profile as prof                            # noqa: E402
from nnr_amd.config import make_config                        # noqa: E402
from nnr_amd.model import Model                               # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch    # noqa: E402
from nnr_amd.trainer import Trainer                           # noqa: E402
from npa_bench import alternate                               # noqa: E402

ENTITY_SIZE = 4000


def with_entities(batch, seed):
    """The batch with entity ids on about a fifth of the title positions (fields 5 and 17: user_title_entity, news_title_entity)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    batch = list(batch)
    for i in (5, 17):
        ids = torch.randint(1, ENTITY_SIZE, batch[i].shape, device='cuda', generator=g, dtype=torch.int32)
        on = torch.rand(batch[i].shape, device='cuda', generator=g) < 0.2
        batch[i] = torch.where(on, ids, torch.zeros_like(ids)).to(batch[i].dtype)
    return batch


def titles_of_a_step(B, V):
    """The batch * 55 titles of one synthetic MIND-shaped batch, candidates then history: word ids / entity ids [n, 32], category, subCategory."""
    b = with_entities(to_torch(SynthCorpus(SynthSpec(vocabulary_size=V)).batch(B, np.random.default_rng(100)), 'cuda'), B)
    cat2 = lambda i, j: torch.cat([b[i].reshape(-1, b[i].shape[-1]), b[j].reshape(-1, b[j].shape[-1])]).contiguous()
    return dict(tt=cat2(15, 3), te=cat2(17, 5), tm=cat2(16, 4).bool(), cat=torch.cat([b[13].reshape(-1), b[1].reshape(-1)]),
                sub=torch.cat([b[14].reshape(-1), b[2].reshape(-1)]))


def build(ne, ue, B, V):
    cfg = make_config(['--news_encoder=' + ne, '--user_encoder=' + ue, '--dataset=200k', '--batch_size=%d' % B],
                      corpus_sizes=dict(vocabulary_size=V, entity_size=ENTITY_SIZE))
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table, torch.randn(ENTITY_SIZE, cfg.entity_embedding_dim) * 0.1, torch.randn(ENTITY_SIZE, cfg.context_embedding_dim) * 0.1)
    model.initialize()
    return cfg, model.cuda().train()


def mode_kernel(a):
    res = {}
    E, C, w, L = 300, 400, 3, 32
    Lp = L + w - 1
    dev = dict(device='cuda', dtype=torch.float32)
    for B in a.batch:
        d = titles_of_a_step(B, a.vocabulary_size)
        n = d['tt'].shape[0]
        g = torch.Generator(device='cuda').manual_seed(B)
        table = torch.randn(a.vocabulary_size, E, generator=g, **dev)
        text = d['tt'].to(torch.int32).reshape(-1).contiguous()
        pre1, pre2 = torch.randn(n * L, E, generator=g, **dev), torch.randn(n * L, E, generator=g, **dev)
        Xp, dXp = torch.empty(n * Lp, 3 * E, **dev), torch.randn(n * Lp, 3 * E, generator=g, **dev)
        outs = [torch.empty(n * L, E, **dev) for _ in range(3)]
        z, bias = torch.randn(n * Lp, C, generator=g, **dev), torch.randn(C, generator=g, **dev)
        out, arg = torch.empty(n, C, **dev), torch.empty(n, C, device='cuda', dtype=torch.uint8)
        dz, db, gup = torch.empty((w - 1) + n * Lp, C, **dev), torch.empty(C, **dev), torch.randn(n, C, generator=g, **dev)
        W, P = torch.randn(C, E, w, 3, generator=g, **dev), torch.empty(C * E * w * 3, **dev)
        ops.window_max_fwd(z, C, bias, n, C, L, w, out, arg)
        v = {'kcnn_image_fwd': lambda i: ops.kcnn_image_fwd(table, text, pre1, pre2, n, L, w, Xp),
             'kcnn_image_bwd': lambda i: ops.kcnn_image_bwd(dXp, Xp, n, L, E, w, *outs),
             'window_max_fwd': lambda i: ops.window_max_fwd(z, C, bias, n, C, L, w, out, arg),
             'window_max_bwd': lambda i: ops.window_max_bwd(gup, arg, n, C, L, w, w - 1, dz, db),
             'kcnn_permute': lambda i: ops.permute(W, P, 'kcnn_p', (C, E, w))}
        t = alternate(v, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(x)) for k, x in t.items()}
        nbytes = {'kcnn_image_fwd': 4.0 * (3 * E * n * Lp + 3 * E * n * L) + 4.0 * n * L, 'kcnn_image_bwd': 4.0 * E * n * L * (3 + 2 + 3),
                  'window_max_fwd': 4.0 * n * (L - w + 1) * C + 5.0 * n * C, 'window_max_bwd': 4.0 * ((w - 1) + n * Lp) * C + 5.0 * n * C,
                  'kcnn_permute': 2 * 4.0 * C * E * w * 3}
        res['batch%d' % B] = {'shape': dict(n=n, L=L, E=E, C=C, w=w), 'ms': t, 'median_ms': med, 'MB': {k: round(x / 1e6, 1) for k, x in nbytes.items()},
                              'GBps': {k: round(nbytes[k] / med[k] / 1e6, 1) for k in med},
                              'share_of_hbm_peak': {k: round(nbytes[k] / med[k] / 1e6 / prof.PEAK_HBM_GBS, 4) for k in med}}
    return res


def kcnn_torch(w, d, L, p):
    """newsEncoders.py:233-240 with layers.py:77-78 in stock torch ops."""
    n = d['tt'].shape[0]
    x0 = F.embedding(d['tt'], w['word'])
    x1 = torch.tanh(F.linear(F.embedding(d['te'], w['entity']), w['M_entity.weight'], w['M_entity.bias']))
    x2 = torch.tanh(F.linear(F.embedding(d['te'], w['context']), w['M_context.weight'], w['M_context.bias']))
    img = torch.stack([x0, x1, x2], dim=3).permute(0, 2, 1, 3)
    win = w['knowledge_cnn.conv.weight'].shape[2]
    c = F.relu(F.conv2d(img, w['knowledge_cnn.conv.weight'], w['knowledge_cnn.conv.bias'], padding=[(win - 1) // 2, 0]))
    rep = torch.max(c[:, :, :L - win + 1], dim=2)[0].view(n, -1)
    return torch.cat([rep, F.dropout(F.embedding(d['cat'], w['cat']), p, True), F.dropout(F.embedding(d['sub'], w['sub']), p, True)], dim=1)


def mode_encoder(a):
    res = {}
    for B in a.batch:
        d = titles_of_a_step(B, a.vocabulary_size)
        d = {k: (v.long() if k in ('tt', 'te', 'cat', 'sub') else v) for k, v in d.items()}
        n, L = d['tt'].shape
        cfg, model = build('KCNN', 'ATT', B, a.vocabulary_size)
        ne = model.news_encoder
        w = {k: v.detach().clone().requires_grad_() for k, v in ne.state_dict().items() if 'embedding' not in k}
        w.update({k: getattr(ne, full).weight.detach().clone().requires_grad_() for k, full in
                  (('word', 'word_embedding'), ('entity', 'entity_embedding'), ('context', 'context_embedding'), ('cat', 'category_embedding'),
                   ('sub', 'subCategory_embedding'))})
        g = torch.Generator(device='cuda').manual_seed(B)
        dout = torch.randn(1, n, ne.news_embedding_dim, device='cuda', generator=g)
        args = (d['tt'].unsqueeze(0), d['tm'].unsqueeze(0), d['te'].unsqueeze(0), None, None, None, d['cat'].unsqueeze(0), d['sub'].unsqueeze(0), None)

        def hip(i):
            (ne(*args) * dout).sum().backward()
            ops.join_extra_streams()

        def ref(i):
            (kcnn_torch(w, d, L, cfg.dropout_rate) * dout[0]).sum().backward()
        ne.eval()
        with torch.no_grad():
            err = float((ne(*args)[0] - kcnn_torch(w, d, L, 0.0)).abs().max())
        ne.train()
        t = alternate({'torch_reference_formulation': ref, 'hip_encoder': hip}, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['batch%d' % B] = {'n': n, 'ms_fwd_bwd': t, 'median_ms': med, 'max_abs_diff_of_outputs_eval': err, 'dropout_rate': cfg.dropout_rate,
                              'speedup': round(med['torch_reference_formulation'] / med['hip_encoder'], 2)}
    return res


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [with_entities(to_torch(corpus.batch(B, rng), 'cuda'), s) for s in range(8)]
    variants, paths, trainers = {}, {}, {}
    for ne, ue in (('CNN', 'CATT'), ('KCNN', 'CATT')):
        cfg, model = build(ne, ue, B, a.vocabulary_size)
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
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
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
