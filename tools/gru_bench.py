#!/usr/bin/env python3
"""Measurements of the GRU user encoder (DAE-GRU) and of the kernels of csrc/gru.hip (profiles/gru_summary.md).  Seeded synthetic data at
DAE-GRU's defaults (history 50 slots, D = 300, H = 200), history lengths from the synthetic MIND-shaped batches (uniform 0 .. 50, a few
empty users).  HIP events around blocks of `--steps` iterations (no device synchronisation inside a block), the variants of a comparison
alternated in one process.

  python tools/gru_bench.py kernel  [--batch 64 8]   every launch of the encoder's forward and backward alone: the projection, the two
                                                     recurrence kernels, the gradient products / column sums, the (un)pack kernels
  python tools/gru_bench.py encoder [--batch 64 8]   the user encoder, forward + backward, vs the reference's formulation in stock torch ops
                                                     (two sorts, the .cpu() length sync, pack_padded_sequence, nn.GRU = the vendor's, dec)
                                                     with torch autograd on the same inputs / weights
  python tools/gru_bench.py step    [--batch 64]     training step of DAE+GRU (autograd path), dropout on, next to DAE+ATT

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib, ops                                  # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch    # noqa: E402
from nnr_amd.trainer import Trainer                           # noqa: E402
from npa_bench import alternate, build                        # noqa: E402

T, D, H = 50, 300, 200


def history(B, V):
    """(history representation stand-in [B, T, D], user_history_mask [B, T]) of one synthetic batch."""
    b = to_torch(SynthCorpus(SynthSpec(vocabulary_size=V)).batch(B, np.random.default_rng(100)), 'cuda')
    g = torch.Generator(device='cuda').manual_seed(B)
    return torch.randn(B, T, D, device='cuda', generator=g), b[9]


def mode_kernel(a):
    res = {}
    f32 = dict(device='cuda', dtype=torch.float32)
    for B in a.batch:
        x, mask = history(B, a.vocabulary_size)
        cfg, model = build('DAE', 'GRU', B, a.vocabulary_size)
        gru = model.user_encoder.gru
        p = gru.param_list()
        w = ops.gru_pack(gru, H, D)
        x2, m8 = x.view(B * T, D), mask.bool().view(torch.uint8).contiguous()
        NP = w.NP
        gates = torch.empty(B * T, NP, **f32)
        hout, hprev, hfinal = torch.zeros(B * T, H, **f32), torch.zeros(B * T, H, **f32), torch.empty(B, H, **f32)
        length = torch.empty(B, device='cuda', dtype=torch.int32)
        dhf = torch.randn(B, H, **f32)
        dw_ihp, dw_hhp, db_p = torch.zeros(NP, D, **f32), torch.zeros(NP, H, **f32), torch.zeros(NP, **f32)
        grads = [torch.zeros_like(t) for t in p]
        ops.linear_fwd(x2, w.w_ihp, w.b_p, out=gates)
        ops.gru_fwd(gates, m8, None, w, B, T, H, hout, hprev, hfinal, length)
        saved = gates.clone()

        def tn(dw, act, K):
            split = ops.split_for(NP, K, B * T) if (K & 3) == 0 else 1
            dw.zero_()
            ops.gemm(gates, act, dw, M=NP, N=K, K=B * T, lda=NP, ldb=K, ldc=K, trans_a=True, trans_b=True, atomic=split > 1, split_k=split)

        def fwd(i):
            ops.linear_fwd(x2, w.w_ihp, w.b_p, out=gates)
            ops.gru_fwd(gates, m8, None, w, B, T, H, hout, hprev, hfinal, length)

        def bwd(i):
            ops.copy_bytes(gates, saved)
            ops.gru_bwd(gates, length, hprev, w, dhf, B, T, H)
        v = {'projection': lambda i: ops.linear_fwd(x2, w.w_ihp, w.b_p, out=gates), 'projection+gru_fwd': fwd,
             'restore+gru_bwd': bwd, 'restore': lambda i: ops.copy_bytes(gates, saved),
             'dX': lambda i: ops.linear_bwd_data(gates, w.w_ihp), 'dW_ih': lambda i: tn(dw_ihp, x2, D), 'dW_hh': lambda i: tn(dw_hhp, hprev, H),
             'bias_sums': lambda i: ops.bias_grad(gates, db_p), 'unpack_grads': lambda i: ops.gru_unpack_grads(dw_ihp, db_p, dw_hhp, H, D, grads),
             'pack_weights': lambda i: w.pack(p)}
        t = alternate(v, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(x)) for k, x in t.items()}
        med['gru_fwd'] = round(med['projection+gru_fwd'] - med['projection'], 4)
        med['gru_bwd'] = round(med['restore+gru_bwd'] - med['restore'], 4)
        lens = length.cpu()
        res['batch%d' % B] = {'shape': dict(B=B, T=T, D=D, H=H, NP=NP, live_slots=int(lens.sum()), longest=int(lens.max()), empty_users=int((lens == 0).sum())),
                              'ms': t, 'median_ms': med, 'us_per_step_fwd': round(1e3 * med['gru_fwd'] / max(1, int(lens.max())), 2),
                              'us_per_step_bwd': round(1e3 * med['gru_bwd'] / max(1, int(lens.max())), 2)}
    return res


def gru_torch(gru, dec, hist, mask, N):
    """The stock formulation of userEncoders.py:301-331: lengths from the mask, sort by length, drop the empty users, pack (the lengths go to the
    host), nn.GRU, dec + tanh, zero rows for the empty users, de-sort, repeat over the candidates."""
    B, _, Dm = hist.shape
    snum, order = torch.sort(mask.sum(dim=1).long(), descending=True)
    back = torch.sort(order)[1]
    live = int((snum > 0).sum())
    user = hist.new_zeros((B, Dm))
    if live:
        packed = pack_padded_sequence(hist.index_select(0, order[:live]), snum[:live].cpu(), batch_first=True)
        user = torch.cat([torch.tanh(dec(gru(packed)[1].squeeze(0))), hist.new_zeros((B - live, Dm))]).index_select(0, back)
    return user.unsqueeze(1).expand(-1, N, -1)


def mode_encoder(a):
    res = {}
    N = 5
    for B in a.batch:
        x, mask = history(B, a.vocabulary_size)
        cfg, model = build('DAE', 'GRU', B, a.vocabulary_size)
        ue = model.user_encoder
        ref_gru = torch.nn.GRU(D, H, batch_first=True).cuda()
        ref_gru.load_state_dict(ue.gru.state_dict(), strict=True)
        ref_dec = torch.nn.Linear(H, D).cuda()
        ref_dec.load_state_dict(ue.dec.state_dict())
        g = torch.Generator(device='cuda').manual_seed(B + 1)
        dout = torch.randn(B, N, D, device='cuda', generator=g)
        cand = torch.empty(B, N, D, device='cuda')
        xh, xr = x.clone().requires_grad_(), x.clone().requires_grad_()

        def hip(i):
            (ue.encode_user(xh, mask, None, None, None, cand) * dout).sum().backward()
            ops.join_extra_streams()

        def ref(i):
            (gru_torch(ref_gru, ref_dec, xr, mask, N) * dout).sum().backward()
        with torch.no_grad():
            err = float((ue.encode_user(x, mask, None, None, None, cand) - gru_torch(ref_gru, ref_dec, x, mask, N)).abs().max())
        t = alternate({'torch_reference_formulation': ref, 'hip_encoder': hip}, a.steps, a.warmup, a.rounds)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res['batch%d' % B] = {'ms_fwd_bwd': t, 'median_ms': med, 'max_abs_diff_of_outputs': err,
                              'ratio_torch_over_hip': round(med['torch_reference_formulation'] / med['hip_encoder'], 2)}
    return res


def mode_step(a):
    B = a.batch[0]
    corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
    rng = np.random.default_rng(100)
    batches = [to_torch(corpus.batch(B, rng), 'cuda') for _ in range(8)]
    variants, paths, trainers = {}, {}, {}
    for ne, ue in (('DAE', 'ATT'), ('DAE', 'GRU')):
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
