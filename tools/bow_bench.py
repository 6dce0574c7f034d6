#!/usr/bin/env python3
"""Measurements of the bag-of-words news encoders DAE and Inception and of the bag kernels (profiles/bow_summary.md).  Seeded synthetic
data, MIND-200k shapes (title 32, abstract 128 slots, batch * 55 news per step), HIP events around blocks of `--steps` iterations (no
device synchronisation inside a block), the variants of a comparison alternated in one process.

  python tools/bow_bench.py kernel  [--batch 64 8]   nnr_bag_mean_fwd and nnr_bag_mean_bwd alone, both modes: duration and achieved share of the
                                                     HBM bandwidth, bytes = table rows of the live positions read + outputs written (forward),
                                                     sorted list + the n gradient rows read + touched table rows read and written (backward)
  python tools/bow_bench.py encoder [--batch 64 8]   one encoder call over the batch's batch * 55 news, forward + backward, dropout on, vs the
                                                     reference's formulation in stock torch ops with torch autograd on the same inputs / weights

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
from npa_bench import alternate                               # noqa: E402


def news_of_a_step(B, V):
    """The batch * 55 news of one synthetic MIND-shaped batch, candidates then history: ids / masks [n, 32], [n, 128], category, subCategory."""
    b = to_torch(SynthCorpus(SynthSpec(vocabulary_size=V)).batch(B, np.random.default_rng(100)), 'cuda')
    cat2 = lambda i, j: torch.cat([b[i].reshape(-1, b[i].shape[-1]), b[j].reshape(-1, b[j].shape[-1])]).contiguous()
    return dict(tt=cat2(15, 3), tm=cat2(16, 4).bool(), ct=cat2(18, 6), cm=cat2(19, 7).bool(), cat=torch.cat([b[13].reshape(-1), b[1].reshape(-1)]),
                sub=torch.cat([b[14].reshape(-1), b[2].reshape(-1)]))


def build(ne, B, V, **over):
    flags = ['--news_encoder=' + ne, '--user_encoder=ATT', '--dataset=200k', '--batch_size=%d' % B] + ['--%s=%s' % kv for kv in over.items()]
    cfg = make_config(flags, corpus_sizes=dict(vocabulary_size=V))
    torch.manual_seed(cfg.seed)
    table = torch.randn(cfg.vocabulary_size, cfg.word_embedding_dim) * 0.3
    table[0] = 0
    model = Model(cfg, table)
    model.initialize()
    return cfg, model.cuda().train()


def mode_kernel(a):
    res = {}
    E = 300
    for B in a.batch:
        d = news_of_a_step(B, a.vocabulary_size)
        n, La, Lb = d['tt'].shape[0], d['tt'].shape[1], d['ct'].shape[1]
        g = torch.Generator(device='cuda').manual_seed(B)
        dev = dict(device='cuda', dtype=torch.float32)
        table = torch.randn(a.vocabulary_size, E, generator=g, **dev)
        tt, ct = d['tt'].to(torch.int32).contiguous(), d['ct'].to(torch.int32).contiguous()
        per = {}
        for mode, separate, act in (('joint_sigmoid', False, ops.ACT_SIGMOID), ('separate_none', True, ops.ACT_NONE)):
            tm, cm = d['tm'].clone(), d['cm'].clone()
            if separate:
                tm[:, 0], cm[:, 0] = True, True
            live = int(tm.sum()) + int(cm.sum())
            words = int(torch.unique(torch.cat([tt[tm], ct[cm]])).numel())
            cols = 2 * E if separate else E
            out, count, dtable = torch.empty((n, cols), **dev), torch.empty(2 * n, **dev), torch.zeros_like(table)
            dout = torch.randn(n, cols, generator=g, **dev)
            plan = ops.BagPlan(n, La, Lb, a.vocabulary_size, torch.device('cuda'))
            ops.bag_mean_fwd(table, tt, tm, ct, cm, separate, act, out, cols, 0, E if separate else 0, count, plan)
            plan.sort()
            torch.cuda.synchronize()
            v = {'bag_mean_fwd': lambda i: ops.bag_mean_fwd(table, tt, tm, ct, cm, separate, act, out, cols, 0, E if separate else 0, count, plan),
                 'bag_mean_bwd': lambda i: ops.bag_mean_bwd(dout, cols, out, cols, 0, E if separate else 0, count, plan, separate, act, dtable)}
            t = alternate(v, a.steps, a.warmup, a.rounds)
            ops.join_extra_streams()
            torch.cuda.synchronize()
            med = {k: float(np.median(x)) for k, x in t.items()}
            fwd_bytes = 4.0 * E * live + 4.0 * n * cols + 5.0 * n * (La + Lb) + 4.0 * n * (La + Lb)
            bwd_bytes = 8.0 * n * (La + Lb) + 4.0 * n * cols * (2 if act == ops.ACT_SIGMOID else 1) + 2 * 4.0 * E * words
            per[mode] = {'ms': t, 'median_ms': med, 'live_positions': live, 'live_fraction': round(live / (n * (La + Lb)), 4), 'distinct_words': words,
                         'GBps': {'fwd': round(fwd_bytes / med['bag_mean_fwd'] / 1e6, 1), 'bwd': round(bwd_bytes / med['bag_mean_bwd'] / 1e6, 1)},
                         'share_of_hbm_peak': {'fwd': round(fwd_bytes / med['bag_mean_fwd'] / 1e6 / prof.PEAK_HBM_GBS, 4),
                                               'bwd': round(bwd_bytes / med['bag_mean_bwd'] / 1e6 / prof.PEAK_HBM_GBS, 4)},
                         'gathered_buffer_bytes_avoided': 2 * 4.0 * E * n * (La + Lb)}
        res['batch%d' % B] = {'shape': dict(n=n, La=La, Lb=Lb, E=E, V=a.vocabulary_size), **per}
    return res


def dae_torch(w, d, Alpha, p):
    """newsEncoders.py:383-394 in stock torch ops (the representation and the auxiliary term)."""
    tm, cm = d['tm'].unsqueeze(2), d['cm'].unsqueeze(2)
    m = torch.sigmoid(((F.embedding(d['tt'], w['word']) * tm).sum(dim=1) + (F.embedding(d['ct'], w['word']) * cm).sum(dim=1)) / (tm.sum(dim=1) + cm.sum(dim=1)))
    h = torch.sigmoid(F.linear(F.dropout(m, p, True), w['f1.weight'], w['f1.bias']))
    dd = torch.sigmoid(F.linear(h, w['f2.weight'], w['f2.bias']))
    aux = torch.norm(m - dd, dim=1) * Alpha
    rep = torch.cat([h, F.dropout(F.embedding(d['cat'], w['cat']), p, True), F.dropout(F.embedding(d['sub'], w['sub']), p, True)], dim=1)
    return rep, aux


def inception_torch(w, d):
    """newsEncoders.py:421-433 in stock torch ops (the masks' position 0 is live already)."""
    tm, cm = d['tm'].unsqueeze(2), d['cm'].unsqueeze(2)
    t = (F.embedding(d['tt'], w['word']) * tm).sum(dim=1) / tm.sum(dim=1)
    c = (F.embedding(d['ct'], w['word']) * cm).sum(dim=1) / cm.sum(dim=1)
    cat, sub = F.embedding(d['cat'], w['cat']), F.embedding(d['sub'], w['sub'])
    e = torch.cat([t, c, cat, sub], dim=1)
    lin = lambda x, k: F.linear(x, w[k + '.weight'], w[k + '.bias'])
    s1 = F.relu(lin(F.relu(lin(F.relu(lin(e, 'fc1_1')), 'fc1_2')), 'fc1_3'))
    s2 = F.relu(lin(e, 'fc2'))
    return lin(torch.cat([s1, s2, t + c + cat + sub], dim=1), 'linear_transform')


def mode_encoder(a):
    res = {}
    for B in a.batch:
        d = news_of_a_step(B, a.vocabulary_size)
        d['tm'][:, 0], d['cm'][:, 0] = True, True                     # (every synthetic news has a word; Inception sets it anyway)
        n = d['tt'].shape[0]
        out = {}
        for name, over in (('DAE', {}), ('Inception', dict(category_embedding_dim=300, subCategory_embedding_dim=300))):
            cfg, model = build(name, B, a.vocabulary_size, **over)
            ne = model.news_encoder
            w = {k: v.detach().clone().requires_grad_() for k, v in ne.state_dict().items() if '.' in k and 'embedding' not in k}
            w.update(word=ne.word_embedding.weight.detach().clone().requires_grad_(), cat=ne.category_embedding.weight.detach().clone().requires_grad_(),
                     sub=ne.subCategory_embedding.weight.detach().clone().requires_grad_())
            g = torch.Generator(device='cuda').manual_seed(B)
            dout = torch.randn(1, n, ne.news_embedding_dim, device='cuda', generator=g)
            args = (d['tt'].unsqueeze(0), d['tm'].unsqueeze(0), None, d['ct'].unsqueeze(0), d['cm'].unsqueeze(0), None, d['cat'].unsqueeze(0),
                    d['sub'].unsqueeze(0), None)

            def hip(i):
                rep = ne(*args)
                loss = (rep * dout).sum()
                if ne.auxiliary_loss is not None:
                    loss = loss + ne.auxiliary_loss.mean()
                loss.backward()
                ops.join_extra_streams()

            def ref(i):
                if name == 'DAE':
                    rep, aux = dae_torch(w, d, cfg.Alpha, cfg.dropout_rate)
                    ((rep * dout[0]).sum() + aux.mean()).backward()
                else:
                    (inception_torch(w, d) * dout[0]).sum().backward()
            ne.eval()
            with torch.no_grad():
                got = ne(*args)[0]
                exp = dae_torch(w, d, cfg.Alpha, 0.0)[0] if name == 'DAE' else inception_torch(w, d)
                err = float((got - exp).abs().max())
            ne.train()
            t = alternate({'torch_reference_formulation': ref, 'hip_encoder': hip}, a.steps, a.warmup, a.rounds)
            med = {k: float(np.median(v)) for k, v in t.items()}
            out[name] = {'ms_fwd_bwd': t, 'median_ms': med, 'max_abs_diff_of_outputs_eval': err, 'dropout_rate': cfg.dropout_rate,
                         'speedup': round(med['torch_reference_formulation'] / med['hip_encoder'], 2)}
        res['batch%d' % B] = {'n': n, **out}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'encoder'])
    ap.add_argument('--batch', type=int, nargs='+', default=[64, 8])
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--vocabulary_size', type=int, default=60000)
    a = ap.parse_args()
    _lib.lib()
    res = {'kernel': mode_kernel, 'encoder': mode_encoder}[a.mode](a)
    print(json.dumps({'mode': a.mode, 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(0), 'steps_per_block': a.steps,
                      'rounds': a.rounds, 'result': res}))


if __name__ == '__main__':
    main()
