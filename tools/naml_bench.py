#!/usr/bin/env python3
"""Measurements of the single-view NAML encoders (profiles/naml_summary.md): the padded-row convolution against CNN's shifted products,
the view-pool kernels against the same math in existing ops, the encoders against the reference's formulation in stock torch ops, and the
training step.  Seeded synthetic data, MIND-200k shapes, HIP events around blocks of `--steps` iterations (no device synchronisation inside
a block), the variants of a comparison alternated in one process.

  python tools/naml_bench.py kernel  [--batch 64]     convolution forward + backward at n = batch * 55 news, L = 32 and L = 128: functional.Conv1dImageFn
                                                      against EmbedDropFn + Conv1dReluFn on the same ids and weights (outputs and gradients compared);
                                                      view attention forward + backward at --batch and at batch 8: functional.ViewPoolFn against stack +
                                                      layers._AttentionFn (L = 3) + per-news affines
  python tools/naml_bench.py encoder [--batch 64 8]   one NAML_Title / NAML_Content call, forward + backward, dropout off, against the reference's
                                                      formulation (variantEncoders.py:126-143) in stock torch ops on the same weights
  python tools/naml_bench.py step    [--batch 64]     training step, dropout on: CNN+ATT, NAML_Title+ATT, NAML_Content+ATT (autograd path), the
                                                      NAML pairs also with the shifted-product convolution

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops, functional as Fn, news_encoders as NE    # noqa: E402
from nnr_amd.config import make_config                        # noqa: E402
from nnr_amd.layers import _AttentionFn, grad_of              # noqa: E402
from nnr_amd.model import Model                               # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch    # noqa: E402
from nnr_amd.trainer import Trainer                           # noqa: E402


def timed(fn, steps):
    """ms per iteration of `steps` back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    ops.join_extra_streams()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternate(variants, steps, warmup, rounds):
    """{name: [ms per iteration, one per round]} with the variants alternated round by round."""
    for fn in variants.values():
        for i in range(warmup):
            fn(i)
    ops.join_extra_streams()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(round(timed(fn, steps), 4))
    return out


def spread(xs):
    return round(float(max(xs) - min(xs)), 4)


def build(ne, ue, batch, V, **over):
    cfg = make_config(['--news_encoder=' + ne, '--user_encoder=' + ue, '--dataset=200k', '--batch_size=%d' % batch],
                      corpus_sizes=dict(vocabulary_size=V), **over)
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table)
    model.initialize()
    return cfg, model.cuda().train()


def zero_grads(mod):
    for q in mod.parameters():
        if q.grad is not None:
            ops.fill_zero(q.grad)


def mode_kernel(a):
    res = {'conv': {}, 'view': {}}
    B = a.batch[0]
    n = B * 55
    for Lx in (32, 128):
        cfg, model = build('NAML_Title' if Lx == 32 else 'NAML_Content', 'ATT', B, a.vocabulary_size)
        ne = model.news_encoder
        conv, table = ne.text_conv().conv, ne.word_embedding.weight
        E, C = cfg.word_embedding_dim, cfg.cnn_kernel_num
        g = torch.Generator(device='cuda').manual_seed(Lx)
        # MIND-shaped ids: frequent small ids, PAD past a news's length
        ids = (torch.rand(n, Lx, device='cuda', generator=g) ** 3 * (a.vocabulary_size - 1)).int() + 1
        lens = torch.randint(1, Lx + 1, (n, 1), device='cuda', generator=g)
        ids = torch.where(torch.arange(Lx, device='cuda')[None, :] < lens, ids, torch.zeros_like(ids)).contiguous()
        dy = torch.randn(n * Lx, C, device='cuda', generator=g)
        p, seed = 0.2, 1234

        def image(i=0):
            y = Fn.Conv1dImageFn.apply(table, ids, conv, n, Lx, p, seed, True)
            y.backward(dy)
            return y

        def shifted(i=0):
            w = Fn.EmbedDropFn.apply(table, ids, p, seed)
            y = Fn.Conv1dReluFn.apply(w, conv, n, Lx)
            y.backward(dy)
            return y
        outs = {}
        for name, fn in (('image', image), ('shifted', shifted)):
            zero_grads(ne)
            y = fn()
            ops.join_extra_streams()
            torch.cuda.synchronize()
            outs[name] = (y.detach().clone(), conv.weight.grad.clone(), conv.bias.grad.clone(), table.grad.clone())
        diff = {k: float((outs['image'][j] - outs['shifted'][j]).abs().max() / outs['shifted'][j].abs().max())
                for j, k in enumerate(('y', 'dweight', 'dbias', 'dtable'))}
        t = alternate({'image': image, 'shifted': shifted}, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['conv']['L%d' % Lx] = {'shape': dict(n=n, L=Lx, E=E, C=C, k=conv.weight.shape[2], p=p), 'ms_fwd_bwd': t, 'median_ms': med,
                                   'spread_ms': {k: spread(v) for k, v in t.items()}, 'speedup': round(med['shifted'] / med['image'], 3),
                                   'max_diff_over_scale': diff}
        del model, outs
        torch.cuda.empty_cache()
    for Bv in sorted(set([B, 8]), reverse=True):
        cfg, model = build('NAML_Title', 'ATT', Bv, 2000)
        ne = model.news_encoder
        nv, C = Bv * 55, cfg.cnn_kernel_num
        g = torch.Generator(device='cuda').manual_seed(Bv)
        text = torch.randn(nv, C, device='cuda', generator=g).requires_grad_()
        cat = torch.randint(0, cfg.category_num, (nv,), device='cuda', generator=g)
        sub = torch.randint(0, cfg.subCategory_num, (nv,), device='cuda', generator=g)
        cat[nv // 2:], sub[nv // 2:] = 0, 0                                 # half of the history slots are PAD news
        dout = torch.randn(nv, C, device='cuda', generator=g)
        att = SimplePool(ne)

        def fused(i=0):
            out = Fn.ViewPoolFn.apply(ne, cat, sub, text)
            out.backward(dout)
            return out

        def existing(i=0):
            a_ = Fn.LinearFn.apply(_RowsFn.apply(ne.category_embedding.weight, cat), ne.category_affine.weight, ne.category_affine.bias, ops.ACT_RELU, 0.0, 0)
            s_ = Fn.LinearFn.apply(_RowsFn.apply(ne.subCategory_embedding.weight, sub), ne.subCategory_affine.weight, ne.subCategory_affine.bias, ops.ACT_RELU, 0.0, 0)
            out = _AttentionFn.apply(torch.stack([text, a_, s_], dim=1), att, None)
            out.backward(dout)
            return out
        zero_grads(ne)
        o1 = fused().detach().clone()
        o2 = existing().detach().clone()
        ops.join_extra_streams()
        torch.cuda.synchronize()
        t = alternate({'view_pool': fused, 'existing_ops': existing}, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['view']['batch%d' % Bv] = {'shape': dict(n=nv, C=C, A=cfg.attention_dim, Ra=cfg.category_num, Rb=cfg.subCategory_num), 'ms_fwd_bwd': t,
                                       'median_ms': med, 'spread_ms': {k: spread(v) for k, v in t.items()},
                                       'speedup': round(med['existing_ops'] / med['view_pool'], 3), 'max_abs_diff_of_outputs': float((o1 - o2).abs().max())}
    return res


class _RowsFn(torch.autograd.Function):
    """table[ids] for a small table through the existing nnr_small_embed kernels (what InceptionFn uses for the category rows)."""

    @staticmethod
    def forward(ctx, table, ids):
        ids = ids.to(torch.int32).contiguous()
        out = torch.empty((ids.numel(), table.shape[1]), device=table.device, dtype=torch.float32)
        ops.small_embed_fwd(table, ids, out, table.shape[1], 0.0, 0)
        ctx.table, ctx.ids = table, ids
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        ops.small_embed_bwd(ctx.ids, dout.shape[1], dout, dout.shape[1], grad_of(ctx.table), 0.0, 0)
        return None, None


class SimplePool:
    """The view attention's affine1 / affine2 presented as a layers.Attention to _AttentionFn."""

    def __init__(self, ne):
        self.affine1, self.affine2 = ne.affine1, ne.affine2


def reference_encoder(ne, text, cat, sub):
    """variantEncoders.py:126-143 in stock torch ops (dropout off)."""
    F = torch.nn.functional
    n = text.shape[0] * text.shape[1]
    conv, att = ne.text_conv().conv, ne.text_attention()
    w = F.embedding(text.reshape(n, -1).long(), ne.word_embedding.weight)
    c = F.relu(F.conv1d(w.permute(0, 2, 1), conv.weight, conv.bias, padding=conv.padding[0])).permute(0, 2, 1)
    al = F.softmax(F.linear(torch.tanh(F.linear(c, att.affine1.weight, att.affine1.bias)), att.affine2.weight).squeeze(2), dim=1)
    t = torch.bmm(al.unsqueeze(1), c).squeeze(1)
    a_ = F.relu(F.linear(F.embedding(cat.reshape(n).long(), ne.category_embedding.weight), ne.category_affine.weight, ne.category_affine.bias))
    s_ = F.relu(F.linear(F.embedding(sub.reshape(n).long(), ne.subCategory_embedding.weight), ne.subCategory_affine.weight, ne.subCategory_affine.bias))
    feat = torch.stack([t, a_, s_], dim=1)
    alpha = F.softmax(F.linear(torch.tanh(F.linear(feat, ne.affine1.weight, ne.affine1.bias)), ne.affine2.weight), dim=1)
    return (feat * alpha).sum(dim=1)


def mode_encoder(a):
    res = {}
    for name in ('NAML_Title', 'NAML_Content'):
        for B in a.batch:
            cfg, model = build(name, 'ATT', B, a.vocabulary_size, dropout_rate=0.0)
            ne = model.news_encoder
            b = to_torch(SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size)).batch(B, np.random.default_rng(100)), 'cuda')
            text = b[3] if name == 'NAML_Title' else b[6]                   # the history call: B * 50 news
            cat, sub = b[1], b[2]
            dout = torch.randn(text.shape[0], text.shape[1], cfg.cnn_kernel_num, device='cuda', generator=torch.Generator(device='cuda').manual_seed(B))

            def hip(i=0):
                rep = ne(b[3], b[4], b[5], b[6], b[7], b[8], cat, sub, None)
                rep.backward(dout)
                return rep

            def ref(i=0):
                rep = reference_encoder(ne, text, cat, sub).view(dout.shape)
                rep.backward(dout)
                return rep
            err = float((hip().detach() - ref().detach()).abs().max())
            t = alternate({'hip': hip, 'torch_reference_formulation': ref}, a.steps, a.warmup, a.rounds)
            med = {k: float(np.median(v)) for k, v in t.items()}
            res['%s_batch%d' % (name, B)] = {'news': text.shape[0] * text.shape[1], 'L': text.shape[2], 'ms_fwd_bwd': t, 'median_ms': med,
                                             'speedup': round(med['torch_reference_formulation'] / med['hip'], 2), 'max_abs_diff_of_outputs': err}
            del model
            torch.cuda.empty_cache()
    return res


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(4)]
    variants, paths, trainers = {}, {}, {}
    for ne in ('CNN', 'NAML_Title', 'NAML_Content'):
        cfg, model = build(ne, 'ATT', B, a.vocabulary_size)
        trainers[ne + '+ATT'] = Trainer(model, cfg)
        variants[ne + '+ATT'] = lambda i, tr=trainers[ne + '+ATT']: tr.train_step(batches[i % len(batches)])
        if ne != 'CNN':
            def shifted(i, tr=trainers[ne + '+ATT']):
                NE.CONV1D_IMAGE = False
                try:
                    tr.train_step(batches[i % len(batches)])
                finally:
                    NE.CONV1D_IMAGE = True
            variants[ne + '+ATT shifted-product convolution'] = shifted
    t = alternate(variants, a.steps, a.warmup, a.rounds)
    for k, tr in trainers.items():
        paths[k] = tr.last_path
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {'batch': B, 'dropout_rate': 0.2, 'ms_per_step': t, 'median_ms': med, 'spread_ms': {k: spread(v) for k, v in t.items()}, 'path': paths}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'encoder', 'step'])
    ap.add_argument('--batch', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--vocabulary_size', type=int, default=60000)
    a = ap.parse_args()
    if a.batch is None:
        a.batch = [64, 8] if a.mode == 'encoder' else [64]
    _lib.lib()
    res = {'kernel': mode_kernel, 'encoder': mode_encoder, 'step': mode_step}[a.mode](a)
    print(json.dumps({'mode': a.mode, 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(0), 'steps_per_block': a.steps,
                      'rounds': a.rounds, 'result': res}))


if __name__ == '__main__':
    main()
