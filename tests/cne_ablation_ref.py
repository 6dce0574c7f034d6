"""Float64 restatement of the news-encoder ablations CNE_Title / CNE_Content / CNE_wo_CS / CNE_wo_CA (variantEncoders.py:14-99,190-339) in
plain torch, written from the math (test infrastructure; tests/test_cne_ablation_host.py pins it to fixtures captured from the reference).

Per stream (title, content), for a call of n news with lengths len_i = sum(mask_i) after mask[:, 0] = 1:
    x_it   = keep_it * E[text_it] / (1 - p)                                   word rows, dropout site 'title' / 'content'
    h_it   = [LSTM_fwd(x_i, 0 .. len_i - 1)_t, LSTM_rev(x_i, len_i - 1 .. 0)_t]   for t < len_i, zero beyond (a packed Bi-LSTM)
    m_i    = [c_fwd at t = len_i - 1, c_rev at t = 0]                         the final cell states
gate (CNE_wo_CA):   g_it = sigmoid(H h_it + M m'_partner(i) + b_M),  h~_it = h_it g_it  -- m' the OTHER stream's memory; the partner of the
    sequence at sorted rank r of this stream is the sequence at sorted rank r of the other stream (pair = 'rank': lengths sorted descending,
    ties in index order) or simply sequence i (pair = 'index': what a per-news pairing would give -- the wrong one, kept as a switch so that a
    test can show the fixture tells the two apart).  The positions t >= len_i of h~ never reach a result: the pools mask them.
self pool:          a_it = w2 . tanh(W1 h~_it + b1),  alpha_i = softmax over t of a_it (masked: -1e9),  self_i = sum_t alpha_it h~_it
cross pool (CNE_wo_CS):  a_it = <K h_it, Q self'_i + b_Q> / sqrt(A) with self' the OTHER stream's self vector; out_i = self_i + cross_i
fusion:             [streams' vectors, keep * category row / (1 - p), keep * subCategory row / (1 - p)]   sites 'cat', 'sub'."""
import math

import numpy as np
import torch

VARIANTS = {'CNE_Title': (('title',), False, False), 'CNE_Content': (('content',), False, False),
            'CNE_wo_CS': (('title', 'content'), False, True), 'CNE_wo_CA': (('title', 'content'), True, False)}


def f64(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).double()


def fixed_mask(mask, L):
    """The mask as the encoder leaves it: a [n, L] bool copy with column 0 set."""
    m = torch.as_tensor(np.asarray(mask) if not torch.is_tensor(mask) else mask).reshape(-1, L).bool().clone()
    m[:, 0] = True
    return m


def bilstm(x, lens, P, pre):
    """x [n, L, E], lens [n] -> (h [n, L, 2H] with zeros beyond each length, c_n [n, 2H])."""
    n, L, _ = x.shape
    H = P[pre + 'weight_hh_l0'].shape[1]
    hs, cn = [], []
    for sfx, reverse in (('', False), ('_reverse', True)):
        Wi, Wh = P[pre + 'weight_ih_l0' + sfx], P[pre + 'weight_hh_l0' + sfx]
        b = P[pre + 'bias_ih_l0' + sfx] + P[pre + 'bias_hh_l0' + sfx]
        h, c = x.new_zeros(n, H), x.new_zeros(n, H)
        out = [None] * L
        for t in (range(L - 1, -1, -1) if reverse else range(L)):
            live = (t < lens).unsqueeze(1)
            z = x[:, t] @ Wi.t() + h @ Wh.t() + b
            i, f, g, o = z[:, :H].sigmoid(), z[:, H:2 * H].sigmoid(), z[:, 2 * H:3 * H].tanh(), z[:, 3 * H:].sigmoid()
            c2 = f * c + i * g
            h2 = o * c2.tanh()
            c, h = torch.where(live, c2, c), torch.where(live, h2, h)
            out[t] = torch.where(live, h2, torch.zeros_like(h2))
        hs.append(torch.stack(out, dim=1))
        cn.append(c)
    return torch.cat(hs, dim=2), torch.cat(cn, dim=1)


def masked_softmax(a, mask):
    return torch.softmax(a.masked_fill(~mask, -1e9), dim=1)


class Encoder:
    """One ablation with the parameters of `state` ({'<prefix><name>': array}) as float64 leaves: call it once per encoder call, then
    grads(reps, douts) gives {'grad/<name>': tensor} of sum(rep * dout) over the calls."""

    def __init__(self, name, state, cfg, prefix='news_encoder.'):
        self.name, self.cfg = name, cfg
        self.streams, self.gate, self.cross = VARIANTS[name]
        self.P = {k[len(prefix):]: f64(v).clone().requires_grad_() for k, v in state.items() if k.startswith(prefix)}

    def __call__(self, title_text, title_mask, content_text, content_mask, category, subCategory, keep=None, p=0.0, pair='rank'):
        cfg, P = self.cfg, self.P
        B, N = np.asarray(category).shape[:2] if not torch.is_tensor(category) else category.shape[:2]
        n, A = B * N, cfg.attention_dim
        keep = keep or {}
        scale = 1.0 / (1.0 - p)
        drop = lambda x, site: x if site not in keep else x * f64(keep[site]).reshape(x.shape) * scale
        inputs = {'title': (title_text, title_mask, cfg.max_title_length), 'content': (content_text, content_mask, cfg.max_abstract_length)}
        S = {}
        for k in self.streams:
            text, mask, L = inputs[k]
            m = fixed_mask(mask, L)
            lens = m.sum(dim=1)
            ids = torch.as_tensor(np.asarray(text) if not torch.is_tensor(text) else text).reshape(n, L).long()
            x = drop(P['word_embedding.weight'][ids], k)
            h, cn = bilstm(x, lens, P, k + '_lstm.')
            order = torch.sort(lens, descending=True, stable=True)[1]
            rank = torch.empty_like(order)
            rank[order] = torch.arange(n)
            S[k] = dict(m=m, h=h, cn=cn, order=order, rank=rank)
        if self.gate:
            for k, o in (('title', 'content'), ('content', 'title')):
                st, ot = S[k], S[o]
                partner = ot['order'][st['rank']] if pair == 'rank' else torch.arange(n)
                assert pair in ('rank', 'index')
                mem = ot['cn'][partner] @ P[k + '_M.weight'].t() + P[k + '_M.bias']
                st['x'] = st['h'] * torch.sigmoid(st['h'] @ P[k + '_H.weight'].t() + mem.unsqueeze(1))
        else:
            for k in self.streams:
                S[k]['x'] = S[k]['h']
        for k in self.streams:
            st = S[k]
            a = torch.tanh(st['x'] @ P[k + '_self_attention.affine1.weight'].t() + P[k + '_self_attention.affine1.bias']) \
                @ P[k + '_self_attention.affine2.weight'].reshape(-1)
            st['self'] = (masked_softmax(a, st['m']).unsqueeze(2) * st['x']).sum(dim=1)
        outs = [S[k]['self'] for k in self.streams]
        if self.cross:
            outs = []
            for k, o in (('title', 'content'), ('content', 'title')):
                st = S[k]
                q = S[o]['self'] @ P[k + '_cross_attention.Q.weight'].t() + P[k + '_cross_attention.Q.bias']
                a = ((st['x'] @ P[k + '_cross_attention.K.weight'].t()) * q.unsqueeze(1)).sum(dim=2) / math.sqrt(float(A))
                outs.append(st['self'] + (masked_softmax(a, st['m']).unsqueeze(2) * st['x']).sum(dim=1))
        cat = torch.as_tensor(np.asarray(category) if not torch.is_tensor(category) else category).reshape(n).long()
        sub = torch.as_tensor(np.asarray(subCategory) if not torch.is_tensor(subCategory) else subCategory).reshape(n).long()
        rep = torch.cat(outs + [drop(P['category_embedding.weight'][cat], 'cat'), drop(P['subCategory_embedding.weight'][sub], 'sub')], dim=1)
        return rep.view(B, N, -1)

    def grads(self, reps, douts):
        for q in self.P.values():
            q.grad = None
        sum((r * f64(d)).sum() for r, d in zip(reps, douts)).backward()
        return {'grad/' + k: (q.grad if q.grad is not None else torch.zeros_like(q)).detach() for k, q in self.P.items()}


def encode_batch(name, state, cfg, batch, keep=None, p=0.0, pair='rank', douts=None, prefix='news_encoder.'):
    """Candidate call and history call of a 21-field batch ({field: array}): dict(cand_rep, hist_rep[, grad/...]).  keep: {(site, call): mask}
    as tests/hip_masks.py:cne_masks returns it."""
    enc = Encoder(name, state, cfg, prefix)
    reps = []
    for call, pre in ((0, 'news'), (1, 'user')):
        kc = {site: m for (site, c), m in (keep or {}).items() if c == call}
        reps.append(enc(batch[pre + '_title_text'], batch[pre + '_title_mask'], batch[pre + '_content_text'], batch[pre + '_content_mask'],
                        batch[pre + '_category'], batch[pre + '_subCategory'], keep=kc, p=p, pair=pair))
    out = dict(cand_rep=reps[0].detach(), hist_rep=reps[1].detach())
    if douts is not None:
        out.update(enc.grads(reps, douts))
    return out
