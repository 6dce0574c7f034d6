#!/usr/bin/env python3
"""Measurements of the news-encoder ablations CNE_Title / CNE_Content / CNE_wo_CS / CNE_wo_CA (profiles/cne_ablation_summary.md).  Seeded
synthetic data, MIND-200k shapes, HIP events around blocks of `--steps` iterations (no device synchronisation inside a block), the variants
of a comparison alternated round by round in one process.

  python tools/cne_ablation_bench.py encoder [--batch 64 8]   forward + backward of each encoder's two calls (forward_pair: candidates and
                                                              history as one packed plan) vs the reference's formulation in stock torch
                                                              ops on the same GPU (sort by length, pack_padded_sequence, nn.LSTM, padded
                                                              [n, L, 2H] rows, masked softmax pools), same weights, dropout off
  python tools/cne_ablation_bench.py step    [--batch 64]     training step, dropout on: each variant + SUE (autograd path) beside CNE+SUE
                                                              (its own native path) in the same session

One JSON line per mode on stdout (with the library's build id)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from nnr_amd import _lib                                      # noqa: E402
from nnr_amd.config import VARIANT_NEWS_ENCODERS              # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch    # noqa: E402
from nnr_amd.trainer import Trainer                           # noqa: E402
from sue_ablation_bench import alternate, summary, build      # noqa: E402


class TorchFormulation(nn.Module):
    """The reference's way of computing an ablation (variantEncoders.py:14-99,190-339), in stock torch modules holding the weights of `enc`."""

    def __init__(self, enc):
        super().__init__()
        self.streams, self.gate, self.cross = enc.cne_streams, enc.cne_gate, enc.cne_cross
        self.L = dict(title=enc.max_title_length, content=enc.max_content_length)
        self.A = enc.attention_dim
        self.word, self.cat, self.sub = enc.word_embedding, enc.category_embedding, enc.subCategory_embedding
        self.enc = enc
        self.lstm = nn.ModuleDict()
        for s in self.streams:
            m = nn.LSTM(enc.word_embedding_dim, enc.hidden_dim, batch_first=True, bidirectional=True)
            m.load_state_dict(getattr(enc, s + '_lstm').state_dict())
            self.lstm[s] = m

    def stream(self, s, text, mask):
        n, L = text.shape[0] * text.shape[1], self.L[s]
        mask = mask.reshape(n, L).clone()
        mask[:, 0] = True
        lens = mask.sum(dim=1)
        slen, order = torch.sort(lens, descending=True)
        back = torch.sort(order)[1]
        x = self.word(text.reshape(n, L)).index_select(0, order)
        h, (_, c) = self.lstm[s](pack_padded_sequence(x, slen.cpu(), batch_first=True))
        h, _ = pad_packed_sequence(h, batch_first=True, total_length=L)
        return dict(mask=mask, h=h, m=torch.cat([c[0], c[1]], dim=1), back=back)

    def forward(self, title_text, title_mask, content_text, content_mask, category, subCategory):
        enc = self.enc
        inputs = dict(title=(title_text, title_mask), content=(content_text, content_mask))
        S = {s: self.stream(s, *inputs[s]) for s in self.streams}
        for s in self.streams:
            st = S[s]
            if self.gate:                                         # both in sorted order: the partner is the other stream's row of the same rank
                o = S['content' if s == 'title' else 'title']
                st['h'] = st['h'] * torch.sigmoid(getattr(enc, s + '_H')(st['h']) + getattr(enc, s + '_M')(o['m']).unsqueeze(1))
            st['x'] = st['h'].index_select(0, st['back'])
        for s in self.streams:
            st, sa = S[s], getattr(enc, s + '_self_attention')
            a = torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(st['x'], sa.affine1.weight, sa.affine1.bias)), sa.affine2.weight).squeeze(2)
            st['self'] = torch.bmm(torch.softmax(a.masked_fill(~st['mask'], -1e9), dim=1).unsqueeze(1), st['x']).squeeze(1)
        outs = [S[s]['self'] for s in self.streams]
        if self.cross:
            outs = []
            for s in self.streams:
                st, ca, o = S[s], getattr(enc, s + '_cross_attention'), S['content' if s == 'title' else 'title']
                a = torch.bmm(ca.K(st['x']), ca.Q(o['self']).unsqueeze(2)).squeeze(2) / math.sqrt(float(self.A))
                outs.append(st['self'] + torch.bmm(torch.softmax(a.masked_fill(~st['mask'], -1e9), dim=1).unsqueeze(1), st['x']).squeeze(1))
        B, N = category.shape
        return torch.cat([torch.cat(outs, dim=1).view(B, N, -1), self.cat(category), self.sub(subCategory)], dim=2)


def mode_encoder(a):
    res = {}
    for B in a.batch:
        corpus = SynthCorpus(SynthSpec(vocabulary_size=a.vocabulary_size))
        b = to_torch(corpus.batch(B, np.random.default_rng(100 + B)), 'cuda')
        cand, hist = (b[15], b[16], b[18], b[19], b[13], b[14]), (b[3], b[4], b[6], b[7], b[1], b[2])
        out = {}
        for name in VARIANT_NEWS_ENCODERS + ['CNE']:
            cfg, model = build(name, 'ATT', B, a.vocabulary_size)
            enc = model.news_encoder
            enc.dropout_rate = 0.0
            g = torch.Generator(device='cuda').manual_seed(B)
            D = enc.news_embedding_dim
            douts = [torch.randn(B, x[0].shape[1], D, device='cuda', generator=g) for x in (cand, hist)]
            variants = {'forward_pair': lambda i, enc=enc, douts=douts: torch.autograd.backward(list(enc.forward_pair(cand, hist)), douts)}
            err = None
            if name != 'CNE':
                ref = TorchFormulation(enc).cuda().train()
                variants['torch_reference_formulation'] = lambda i, ref=ref, douts=douts: torch.autograd.backward([ref(*cand), ref(*hist)], douts)
                with torch.no_grad():
                    got = enc.forward_pair(tuple(t.clone() for t in cand), tuple(t.clone() for t in hist))
                    err = max(float((x - y).abs().max()) for x, y in zip(got, (ref(*cand), ref(*hist))))
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
    for ne in VARIANT_NEWS_ENCODERS + ['CNE']:
        cfg, model = build(ne, 'SUE', B, a.vocabulary_size)
        trainers[ne] = Trainer(model, cfg)
        variants[ne + '+SUE'] = (lambda tr: lambda i: tr.train_step(batches[i % len(batches)]))(trainers[ne])
    t = alternate(variants, a.steps, a.warmup, a.rounds)
    return {'batch': B, 'dropout_rate': 0.2, 'ms_per_step': t, 'summary': summary(t), 'path': {k + '+SUE': tr.last_path for k, tr in trainers.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['encoder', 'step'])
    ap.add_argument('--batch', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--vocabulary_size', type=int, default=60000)
    a = ap.parse_args()
    if a.batch is None:
        a.batch = [64] if a.mode == 'step' else [64, 8]
    _lib.lib()
    res = {'encoder': mode_encoder, 'step': mode_step}[a.mode](a)
    print(json.dumps({'mode': a.mode, 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(0), 'steps_per_block': a.steps,
                      'rounds': a.rounds, 'result': res}))


if __name__ == '__main__':
    main()
