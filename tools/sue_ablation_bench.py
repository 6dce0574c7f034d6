#!/usr/bin/env python3
"""Measurements of the user-encoder ablations SUE_wo_GCN / SUE_wo_HCA (profiles/sue_ablation_summary.md).  Seeded synthetic data, MIND-200k
shapes, HIP events around blocks of `--steps` iterations (no device synchronisation inside a block), the variants of a comparison alternated
round by round in one process.

  python tools/sue_ablation_bench.py kernel  [--batch 64 8]   the intra-cluster stage both ways, forward + backward, same inputs: GEMV form
                                                              (u = q W_K, sue_seg_pool_fwd / _bwd, dq = du W_K^T, dW_K += q^T du) vs keys form
                                                              (K projection over the B Hn history rows, sue_intra_fwd / _bwd, the dkf -> dx data
                                                              gradient and the K weight gradient over the same rows)
  python tools/sue_ablation_bench.py encoder [--batch 64 8]   forward + backward of each encoder vs the reference's formulation in stock torch
                                                              ops, and SUE_wo_GCN's whole pipeline with the intra stage in either form (the
                                                              decision rule of the summary reads these two)
  python tools/sue_ablation_bench.py step    [--batch 64]     training step, dropout on: CNE+SUE_wo_GCN, CNE+SUE_wo_HCA (autograd path) and
                                                              CNE+SUE (its own native path)

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops                                 # noqa: E402
from nnr_amd.config import make_config                        # noqa: E402
from nnr_amd.layers import grad_of                            # noqa: E402
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


def summary(t):
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in t.items()}


def build(ne, ue, batch, V):
    cfg = make_config(['--news_encoder=' + ne, '--user_encoder=' + ue, '--dataset=200k', '--batch_size=%d' % batch], corpus_sizes=dict(vocabulary_size=V))
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table)
    model.initialize()
    return cfg, model.cuda().train()


def user_inputs(cfg, B, D, seed):
    """History / candidate representations and the graph, cluster mask and cluster indices of a synthetic batch."""
    corpus = SynthCorpus(SynthSpec(vocabulary_size=2000))
    b = corpus.batch(B, np.random.default_rng(seed))
    g = torch.Generator(device='cuda').manual_seed(seed)
    H, N = cfg.max_history_num, cfg.negative_sample_num + 1
    t = lambda k: torch.from_numpy(np.array(b[k], copy=True)).cuda()
    return dict(hist=0.5 * torch.randn(B, H, D, device='cuda', generator=g), cand=0.5 * torch.randn(B, N, D, device='cuda', generator=g),
                dout=torch.randn(B, N, D, device='cuda', generator=g), hmask=t('user_history_mask'), graph=t('user_history_graph'),
                cmask=t('user_history_category_mask'), cidx=t('user_history_category_indices'))


# ------------------------------------------------------------------------------------------------ the intra stage, both ways
def intra_gemv(mod, x, qc, cidx, dfeat, B, N, Hn, Cn, A, D):
    f32 = dict(device=x.device, dtype=torch.float32)
    Wk, scale = mod.intraCluster_K.weight, 1.0 / math.sqrt(A)
    u = torch.empty((B * N, D), **f32)
    ops.gemm(qc, Wk, u, M=B * N, N=D, K=A, lda=A, ldb=D, ldc=D, trans_b=True)
    alpha, feat = torch.empty((B, N, Hn), **f32), torch.empty((B * N * Cn, D), **f32)
    ops.sue_seg_pool_fwd(x, u, cidx, B, N, Hn, Cn, D, scale, alpha, feat)
    if dfeat is None:
        return feat
    dx, du, dqc = torch.empty((B, Hn, D), **f32), torch.empty((B * N, D), **f32), torch.empty((B * N, A), **f32)
    ops.sue_seg_pool_bwd(x, u, cidx, alpha, dfeat, B, N, Hn, Cn, D, scale, dx, du)
    ops.gemm(du, Wk, dqc, M=B * N, N=A, K=D, lda=D, ldb=D, ldc=A)
    ops.linear_bwd_weight(qc, du, grad_of(Wk))
    return feat, dx, dqc


def intra_keys(mod, x, qc, cidx, dfeat, B, N, Hn, Cn, A, D):
    """The same math through the [B Hn, A] key buffer (the bias, which cancels, left out): SUE's own launches."""
    f32 = dict(device=x.device, dtype=torch.float32)
    Wk = mod.intraCluster_K.weight
    kf = ops.linear_fwd(x.view(B * Hn, D), Wk)
    alpha, feat = torch.empty((B, N, Hn), **f32), torch.empty((B * N * Cn, D), **f32)
    ops.sue_intra_fwd(kf, qc, x, cidx, B, N, Hn, Cn, A, D, alpha, feat)
    if dfeat is None:
        return feat
    dx, dkf, dqc = torch.empty((B, Hn, D), **f32), torch.empty((B * Hn, A), **f32), torch.empty((B * N, A), **f32)
    ops.sue_intra_bwd(kf, qc, x, cidx, alpha, dfeat, B, N, Hn, Cn, A, D, dx, dkf, dqc)
    ops.linear_bwd_data(dkf, Wk, out=dx.view(B * Hn, D), accumulate=True)
    ops.linear_bwd_weight(dkf, x.view(B * Hn, D), grad_of(Wk))
    return feat, dx, dqc


def wo_gcn_pipeline(mod, inp, form):
    """SUE_wo_GCN forward + backward through user_encoders' own stages (dropout off, one stream, weight gradients in line), with the intra stage
    in the given form (user_encoders._IntraGemv / _IntraKeys)."""
    from nnr_amd import user_encoders as UE
    mod.intra_form = form
    try:
        out, sv = UE._cluster_fwd(mod, inp['hist'], inp['cand'], inp['cmask'], inp['cidx'], None, lambda sv: sv['hist'])
        with ops.leaf_scope(out.device, enable=False) as leaf:
            dx, dcand = UE._cluster_bwd(mod, sv, inp['dout'], leaf, None)
    finally:
        del mod.intra_form                                        # (back to the class attribute)
    return out, dx, dcand


# ------------------------------------------------------------------------------------------------ the reference's formulation, stock torch ops
def torch_wo_gcn(mod, inp):
    """variantEncoders.py:369-390 with torch_scatter's two calls as index_add composites."""
    x, c, cidx = inp['hist'], inp['cand'], inp['cidx']
    B, H, D = x.shape
    N, C, A = c.shape[1], mod.category_num, mod.attention_dim
    mask = inp['cmask'].bool().clone()
    mask[:, -1] = True
    he = x.unsqueeze(1).expand(-1, N, -1, -1)
    K = mod.intraCluster_K(he).reshape(B * N, H, A)
    Q = mod.intraCluster_Q(c).view(B * N, A, 1)
    a = torch.bmm(K, Q).view(B, N, H) / math.sqrt(A)
    idx = cidx.unsqueeze(1).expand(-1, N, -1)
    m = torch.full((B, N, C), -math.inf, device=x.device).scatter_reduce(2, idx, a, 'amax', include_self=True)
    e = torch.exp(a - m.gather(2, idx))
    alpha = e / torch.zeros((B, N, C), device=x.device).scatter_add(2, idx, e).gather(2, idx)
    feat = torch.zeros((B, N, C, D), device=x.device).scatter_add(2, idx.unsqueeze(3).expand(-1, -1, -1, D), alpha.unsqueeze(3) * he)
    feat = torch.relu(mod.clusterFeatureAffine(feat)) + feat
    ia = mod.interClusterAttention
    s = torch.bmm(ia.K(feat.view(B * N, C, D)), ia.Q(c.reshape(B * N, D)).unsqueeze(2)).squeeze(2) / math.sqrt(A)
    al = torch.softmax(s.masked_fill(~mask.unsqueeze(1).expand(-1, N, -1).reshape(B * N, C), -1e9), dim=1)
    return torch.bmm(al.unsqueeze(1), feat.view(B * N, C, D)).squeeze(1).view(B, N, D)


def torch_wo_hca(mod, inp):
    """variantEncoders.py:414-418 (dropout off)."""
    x, graph = inp['hist'], inp['graph']
    B, H, D = x.shape
    x0 = torch.cat([x, mod.proxy_node_embedding.unsqueeze(0).expand(B, -1, -1)], dim=1)
    out = x0
    for layer in mod.gcn.gcn_layers:
        y = torch.relu(torch.nn.functional.linear(torch.bmm(graph, out), layer.W.weight, layer.W.bias))
        out = y + out if mod.gcn.residual else y
    gf = (out + x0)[:, :H]
    att = mod.attention
    a = torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(gf, att.affine1.weight, att.affine1.bias)), att.affine2.weight).squeeze(2)
    return torch.bmm(torch.softmax(a, dim=1).unsqueeze(1), gf).squeeze(1).unsqueeze(1).repeat(1, inp['cand'].shape[1], 1)


def mode_kernel(a):
    res = {}
    for B in a.batch:
        D = a.dim or 900                                          # CNE's news_embedding_dim at the 200k defaults
        cfg2, model2 = build_dim(B, D)
        mod = model2.user_encoder
        inp = user_inputs(cfg2, B, D, 100 + B)
        Hn, N, Cn, A = cfg2.max_history_num, cfg2.negative_sample_num + 1, mod.category_num, mod.attention_dim
        qc = ops.linear_fwd(inp['cand'].view(B * N, D), mod.intraCluster_Q.weight, mod.intraCluster_Q.bias)
        dfeat = torch.randn(B * N * Cn, D, device='cuda', generator=torch.Generator(device='cuda').manual_seed(B))
        args = (mod, inp['hist'], qc, inp['cidx'], dfeat, B, N, Hn, Cn, A, D)
        g, k = intra_gemv(*args), intra_keys(*args)
        diff = {n: float((x - y).abs().max()) for n, x, y in zip(('feat', 'dx', 'dqc'), g, k)}
        t = alternate({'gemv_form': lambda i: intra_gemv(*args), 'keys_form': lambda i: intra_keys(*args)}, a.steps, a.warmup, a.rounds)
        res['batch%d' % B] = {'ms_fwd_bwd': t, 'summary': summary(t), 'max_abs_diff': diff, 'shape': dict(B=B, N=N, Hn=Hn, C=Cn, A=A, D=D)}
    return res


def build_dim(B, D):
    """CNN + SUE_wo_GCN with cnn_kernel_num chosen so that news_embedding_dim = D (CNN: kernels + the two 50-wide category embeddings)."""
    cfg = make_config(['--news_encoder=CNN', '--user_encoder=SUE_wo_GCN', '--dataset=200k', '--batch_size=%d' % B, '--cnn_kernel_num=%d' % (D - 100)],
                      corpus_sizes=dict(vocabulary_size=2000))
    torch.manual_seed(cfg.seed)
    model = Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))
    model.initialize()
    assert model.news_embedding_dim == D, model.news_embedding_dim
    return cfg, model.cuda().train()


def mode_encoder(a):
    from nnr_amd import user_encoders as UE
    res = {}
    D = a.dim or 900
    for B in a.batch:
        cfg, model = build_dim(B, D)
        cfg.dropout_rate = 0.0
        out = {}
        for name, ref_fn in (('SUE_wo_GCN', torch_wo_gcn), ('SUE_wo_HCA', torch_wo_hca)):
            torch.manual_seed(3)
            mod = getattr(UE, name)(model.news_encoder, cfg)
            mod.initialize()
            mod = mod.cuda().train()
            inp = user_inputs(cfg, B, D, 200 + B)
            h, c = inp['hist'].requires_grad_(), inp['cand'].requires_grad_()
            ref_mod = getattr(UE, name)(model.news_encoder, cfg).cuda()
            ref_mod.load_state_dict(mod.state_dict())

            def ours(i, mod=mod, inp=inp, h=h, c=c):
                mod.encode_user(h, inp['hmask'], inp['graph'], inp['cmask'].clone(), inp['cidx'], c).backward(inp['dout'])

            def ref(i, ref_mod=ref_mod, inp=inp, ref_fn=ref_fn):
                ref_fn(ref_mod, inp).backward(inp['dout'])
            with torch.no_grad():
                err = float((ref_fn(ref_mod, inp) - mod.encode_user(h, inp['hmask'], inp['graph'], inp['cmask'].clone(), inp['cidx'], c)).abs().max())
            variants = {'torch_reference_formulation': ref, 'encode_user': ours}
            if name == 'SUE_wo_GCN':
                variants['pipeline_gemv_form'] = lambda i, mod=mod, inp=inp: wo_gcn_pipeline(mod, inp, UE._IntraGemv)
                variants['pipeline_keys_form'] = lambda i, mod=mod, inp=inp: wo_gcn_pipeline(mod, inp, UE._IntraKeys)
            t = alternate(variants, a.steps, a.warmup, a.rounds)
            out[name] = {'ms_fwd_bwd': t, 'summary': summary(t), 'max_abs_diff_of_outputs': err}
        res['batch%d' % B] = out
    return res


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(8)]
    variants, trainers = {}, {}
    for ue in ('SUE_wo_GCN', 'SUE_wo_HCA', 'SUE'):
        cfg, model = build('CNE', ue, B, a.vocabulary_size)
        trainers[ue] = Trainer(model, cfg)
        variants['CNE+' + ue] = (lambda tr: lambda i: tr.train_step(batches[i % len(batches)]))(trainers[ue])
    t = alternate(variants, a.steps, a.warmup, a.rounds)
    return {'batch': B, 'dropout_rate': 0.2, 'ms_per_step': t, 'summary': summary(t), 'path': {'CNE+' + k: tr.last_path for k, tr in trainers.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'encoder', 'step'])
    ap.add_argument('--batch', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dim', type=int, default=0, help='news_embedding_dim of the kernel / encoder modes (default 900, CNE at the 200k defaults)')
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
