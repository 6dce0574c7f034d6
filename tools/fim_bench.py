#!/usr/bin/env python3
"""Measurements of the FIM baseline (HDC news encoder + FIM user encoder + FIM click head) and of the kernels of csrc/fim.hip and
csrc/hdc.hip (profiles/fim_summary.md).  Seeded synthetic data, MIND-200k shapes (title 32 slots -> S = 34, 5 candidates, 50 history slots,
E 300, F 150, Conv3d 4 -> 32 -> 16 with kernel 3, MaxPool3d 3 / 3).  HIP events around blocks of `--steps` iterations (no device
synchronisation inside a block), the variants of a comparison alternated in one process.

  python tools/fim_bench.py kernel  [--batch 64 8]   the kernels alone: duration; for the two fused convolution layers the achieved fp32 rate
                                                     (2 Cin K^3 flops per computed position and filter) against the vector fp32 peak
  python tools/fim_bench.py encoder [--batch 64 8]   both news-encoder calls + the user encoder + the head, forward + backward, against the
                                                     reference's formulation in stock torch ops (F.conv1d / F.layer_norm / torch.matmul /
                                                     F.conv3d / F.max_pool3d) with torch autograd on the same inputs and weights
  python tools/fim_bench.py step    [--batch 64]     training step of HDC+FIM (autograd path)

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops                                  # noqa: E402
from nnr_amd.config import make_config                        # noqa: E402
from nnr_amd.model import Model, negative_log_softmax         # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch    # noqa: E402
from nnr_amd.trainer import Trainer                           # noqa: E402
from npa_bench import alternate                               # noqa: E402

PEAK_FP32_VECTOR_TFLOPS = 157.3       # MI355X, packed fp32 FMA; plain v_fma_f32 issues half of it


def build(B, V):
    cfg = make_config(['--news_encoder=HDC', '--user_encoder=FIM', '--click_predictor=FIM', '--dataset=200k', '--batch_size=%d' % B],
                      corpus_sizes=dict(vocabulary_size=V))
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table)
    model.initialize()
    return cfg, model.cuda().train()


def mode_kernel(a):
    res = {}
    S, H, N, E, Fn, F1, F2, K, P, St = 34, 50, 5, 300, 150, 32, 16, 3, 3, 3
    dev = dict(device='cuda', dtype=torch.float32)
    for B in a.batch:
        g = torch.Generator(device='cuda').manual_seed(B)
        imgs, plane = B * N, B * N * S * H * S
        img = torch.randn(4, plane, generator=g, **dev)
        wa, ba = torch.randn(F1, 4, K, K, K, generator=g, **dev) * 0.1, torch.randn(F1, generator=g, **dev) * 0.1
        wb, bb = torch.randn(F2, F1, K, K, K, generator=g, **dev) * 0.03, torch.randn(F2, generator=g, **dev) * 0.1
        sa = (S * H * S, plane, S, H * S, 1)
        da = ops.conv3d_pool_dims(4, H, S, S, F1, K, P, St)
        db = ops.conv3d_pool_dims(F1, da[0], da[1], da[2], F2, K, P, St)
        ca, cb = da[0] * da[1] * da[2], db[0] * db[1] * db[2]
        y1, a1 = torch.empty(imgs, ca, F1, **dev), torch.empty(imgs, ca, F1, device='cuda', dtype=torch.uint8)
        y2, a2 = torch.empty(imgs, F2 * cb, **dev), torch.empty(imgs, F2 * cb, device='cuda', dtype=torch.uint8)
        sb = (ca * F1, 1, da[1] * da[2] * F1, da[2] * F1, F1)
        wpa, wpb, wqa, wqb = ops.conv3d_weight(wa, 0), ops.conv3d_weight(wb, 0), ops.conv3d_weight(wa, 1), ops.conv3d_weight(wb, 1)
        ops.conv3d_pool_fwd(img, sa, wpa, ba, imgs, 4, H, S, S, F1, K, P, St, False, y1, a1)
        ops.conv3d_pool_fwd(y1, sb, wpb, bb, imgs, F1, da[0], da[1], da[2], F2, K, P, St, True, y2, a2)
        dy2, dy1, dimg = torch.randn_like(y2), torch.empty_like(y1), torch.empty_like(img)
        gwa, gba, gwb, gbb = torch.zeros_like(wa), torch.zeros_like(ba), torch.zeros_like(wb), torch.zeros_like(bb)
        c0, h0 = torch.randn(B * N, S, E, generator=g, **dev), torch.randn(B * H, S, E, generator=g, **dev)
        c1, h1 = torch.randn(B * N, S, Fn, generator=g, **dev), torch.randn(B * H, S, Fn, generator=g, **dev)
        dc0, dh0 = torch.empty_like(c0), torch.empty_like(h0)
        n = B * (N + H)
        z, gam, bet = torch.randn(n * (S + 2), Fn, generator=g, **dev), torch.randn(Fn, S, generator=g, **dev), torch.randn(Fn, S, generator=g, **dev)
        y, yp, stats = torch.empty(n, S, Fn, **dev), torch.empty(n * (S + 4), Fn, **dev), torch.empty(n, 2, **dev)
        v = {'conv3d_pool_fwd_a': lambda i: ops.conv3d_pool_fwd(img, sa, wpa, ba, imgs, 4, H, S, S, F1, K, P, St, False, y1, a1),
             'conv3d_pool_fwd_b': lambda i: ops.conv3d_pool_fwd(y1, sb, wpb, bb, imgs, F1, da[0], da[1], da[2], F2, K, P, St, True, y2, a2),
             'conv3d_pool_bwd_b': lambda i: ops.conv3d_pool_bwd(dy2, y2, a2, y1, sb, wqb, imgs, F1, da[0], da[1], da[2], F2, K, P, St, True, dy1, gwb, gbb),
             'conv3d_pool_bwd_a': lambda i: ops.conv3d_pool_bwd(dy1, y1, a1, img, sa, wqa, imgs, 4, H, S, S, F1, K, P, St, False, dimg, gwa, gba),
             'conv3d_pool_bwd_a_weights_only': lambda i: ops.conv3d_pool_bwd(dy1, y1, a1, img, sa, wqa, imgs, 4, H, S, S, F1, K, P, St, False, None, gwa, gba),
             'images_level0_fwd': lambda i: ops.match_images_fwd(c0, h0, B, N, H, S, 0.08, img[0]),
             'images_level1_fwd': lambda i: ops.match_images_fwd(c1, h1, B, N, H, S, 0.08, img[1]),
             'images_level0_bwd': lambda i: ops.match_images_bwd(img[0], c0, h0, B, N, H, S, 0.08, dc0, dh0),
             'ln_relu_fwd': lambda i: ops.hdc_ln_relu_fwd(z, S + 2, gam, bet, n, S, Fn, 1e-5, y, yp, 2, stats)}
        t = alternate(v, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(x)) for k, x in t.items()}
        flops = {'conv3d_pool_fwd_a': 2.0 * imgs * ca * P ** 3 * F1 * 4 * K ** 3, 'conv3d_pool_fwd_b': 2.0 * imgs * cb * P ** 3 * F2 * F1 * K ** 3,
                 'images_level0_fwd': 2.0 * B * N * S * H * S * E, 'images_level1_fwd': 2.0 * B * N * S * H * S * Fn}
        res['batch%d' % B] = {'ms': t, 'median_ms': med, 'GFLOP': {k: round(x / 1e9, 2) for k, x in flops.items()},
                              'TFLOPs': {k: round(flops[k] / med[k] / 1e9, 2) for k in flops},
                              'share_of_fp32_vector_peak': {k: round(flops[k] / med[k] / 1e9 / PEAK_FP32_VECTOR_TFLOPS, 4) for k in flops}}
    return res


def fim_torch(w, b, cfg):
    """newsEncoders.py:262-278, userEncoders.py:244-262 and model.py:131-132 in stock torch ops; b: the 21 batch tensors."""
    def hdc(text, cat, sub):
        Bn, n, L = text.shape
        d0 = torch.cat([F.embedding(cat, w['news_encoder.category_embedding.weight']).unsqueeze(3),
                        F.embedding(sub, w['news_encoder.subCategory_embedding.weight']).unsqueeze(3),
                        F.embedding(text, w['news_encoder.word_embedding.weight']).permute(0, 1, 3, 2)], dim=3)
        x = d0.view(Bn * n, -1, L + 2)
        out = []
        for l in (1, 2, 3):
            x = F.conv1d(x, w['news_encoder.dilated_conv%d.weight' % l], w['news_encoder.dilated_conv%d.bias' % l], padding=l, dilation=l)
            g = w['news_encoder.layer_norm%d.weight' % l]
            x = F.relu(F.layer_norm(x, list(g.shape), g, w['news_encoder.layer_norm%d.bias' % l], 1e-5))
            out.append(x)
        return d0, torch.stack(out, dim=1).view(Bn, n, 3, -1, L + 2)
    c0, cL = hdc(b[15].long(), b[13].long(), b[14].long())
    h0, hL = hdc(b[3].long(), b[1].long(), b[2].long())
    B, N = c0.shape[:2]
    H, S = h0.shape[1], h0.shape[3]
    scalar = math.sqrt(float(cfg.HDC_filter_num))
    m0 = torch.matmul(c0.unsqueeze(2).permute(0, 1, 2, 4, 3), h0.unsqueeze(1)) / scalar
    mL = torch.matmul(cL.unsqueeze(2).permute(0, 1, 2, 3, 5, 4), hL.unsqueeze(1)) / scalar
    img = torch.cat([m0.unsqueeze(3), mL], dim=3).permute(0, 1, 3, 2, 4, 5).reshape(B * N, 4, H, S, S)
    P, St = cfg.maxpooling3D_size, cfg.maxpooling3D_stride
    q = F.max_pool3d(F.elu(F.conv3d(img, w['user_encoder.conv_3D_a.weight'], w['user_encoder.conv_3D_a.bias'])), P, St)
    q = F.max_pool3d(F.elu(F.conv3d(q, w['user_encoder.conv_3D_b.weight'], w['user_encoder.conv_3D_b.bias'])), P, St)
    return F.linear(q.view(B, N, -1), w['fc.weight'], w['fc.bias']).squeeze(2)


def mode_encoder(a):
    res = {}
    for B in a.batch:
        cfg, model = build(B, a.vocabulary_size)
        batch = to_torch(SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size)).batch(B, np.random.default_rng(100)), 'cuda')
        w = {k: p.detach().clone().requires_grad_() for k, p in model.named_parameters()}

        def hip(i):
            negative_log_softmax(model(*batch)).backward()
            ops.join_extra_streams()

        def ref(i):
            lg = fim_torch(w, batch, cfg)
            (-torch.log_softmax(lg, dim=1)[:, 0]).mean().backward()
        with torch.no_grad():
            err = float((model(*batch) - fim_torch(w, batch, cfg)).abs().max())
        t = alternate({'torch_reference_formulation': ref, 'hip_path': hip}, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['batch%d' % B] = {'ms_fwd_bwd': t, 'median_ms': med, 'max_abs_diff_of_logits': err,
                              'speedup': round(med['torch_reference_formulation'] / med['hip_path'], 2)}
    return res


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(4)]
    cfg, model = build(B, a.vocabulary_size)
    tr = Trainer(model, cfg)
    t = alternate({'HDC+FIM': lambda i: tr.train_step(batches[i % len(batches)])}, a.steps, a.warmup, a.rounds)
    return {'batch': B, 'ms_per_step': t, 'median_ms': {k: float(np.median(v)) for k, v in t.items()}, 'path': tr.last_path}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'encoder', 'step'])
    ap.add_argument('--batch', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
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
