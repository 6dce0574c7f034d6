"""float64 restatements for the bag-of-words news encoders DAE and Inception (test infrastructure; the oracle package has neither), written
from the formulas:

  bag_mean   out[r] = act(sum over the live positions of the row's streams of table[id] / count)   -- joint: one mean over both streams;
             separate: one mean per stream, after position 0 of each stream is made live
  row_dist   aux[r] = coef * ||a[r] - b[r]||_2
  linear     y = keep / (1 - p) * act(x W^T + b)
  DAE        m = bag(joint, sigmoid); c = keep / (1 - p) * m; h = sigmoid(f1 c); d = sigmoid(f2 h); aux = Alpha * ||m - d||;
             rep = [h | dropped category row | dropped subCategory row]
  Inception  e = [title mean | abstract mean | category row | subCategory row]; s1 = relu(fc1_3 relu(fc1_2 relu(fc1_1 e))); s2 = relu(fc2 e);
             s3 = the sum of the four slices; rep = linear_transform [s1 | s2 | s3]
  model      candidate call, history call, the ATT (unmasked additive pool) or CATT (tests/cand_attn_ref.py) user encoder, dot-product
             logits, loss = -log_softmax(logits)[:, 0].mean() + the HISTORY call's aux.mean() for DAE (the attribute holds the last call's value)

Everything is torch float64 with autograd on, so the backward pass is the exact derivative of these formulas.  tests/test_bow_host.py pins the
encoders and the model to the reference through tests/golden."""
import numpy as np
import torch

from cand_attn_ref import concat_form


def f64(x):
    return torch.as_tensor(np.asarray(x)).double() if not torch.is_tensor(x) else x.detach().cpu().double()


def _int(x):
    return (torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x.detach().cpu()).long()


def _live(mask, force_first):
    m = (torch.as_tensor(np.asarray(mask)) if not torch.is_tensor(mask) else mask.detach().cpu()) != 0
    if force_first:
        m = m.clone()
        m[:, 0] = True
    return m


def _masked_sum(table, ids, live):
    live = live.to(table.dtype)
    return (table[_int(ids)] * live.unsqueeze(2)).sum(dim=1), live.sum(dim=1, keepdim=True)


def bag_mean(table, ids_a, mask_a, ids_b=None, mask_b=None, separate=False, sigmoid=False):
    """table [V, E] (float64, may require grad; the GPU tests also evaluate it in float32 to size their bars), ids / masks [n, L].  joint: [n, E]; separate: ([n, E] of stream a, [n, E] of stream b or
    None), position 0 of each stream forced live."""
    act = torch.sigmoid if sigmoid else (lambda x: x)
    sa, ca = _masked_sum(table, ids_a, _live(mask_a, separate))
    if ids_b is None:
        return act(sa / ca) if not separate else (act(sa / ca), None)
    sb, cb = _masked_sum(table, ids_b, _live(mask_b, separate))
    if separate:
        return act(sa / ca), act(sb / cb)
    return act((sa + sb) / (ca + cb))


def row_dist(a, b, coef):
    return coef * (a - b).pow(2).sum(dim=1).sqrt()


def _drop(x, keep, p):
    if keep is None or p <= 0.0:
        return x
    keep = keep if torch.is_tensor(keep) else torch.as_tensor(np.asarray(keep))
    return x * keep.detach().cpu().reshape(x.shape).to(x.dtype) / (1.0 - p)


def linear(x, w, b, act=None, keep=None, p=0.0):
    y = x @ w.t() + (b if b is not None else 0.0)
    y = {None: lambda v: v, 'relu': torch.relu, 'sigmoid': torch.sigmoid}[act](y)
    return _drop(y, keep, p)


def dae_call(st, title_text, title_mask, content_text, content_mask, category, subCategory, Alpha, p=0.0, keep=None, pre='news_encoder.'):
    """One DAE call on [B, N, L] inputs with the float64 state `st` {name: tensor} -> (rep [B, N, D], aux [B, N], m [B * N, E]).
    keep: {'corrupt': [n, E], 'cat': [n, cd], 'sub': [n, sd]} keep-masks of the three dropout sites (train mode, p > 0)."""
    B, N, La = np.asarray(title_text).shape if not torch.is_tensor(title_text) else title_text.shape
    n = B * N
    keep = keep or {}
    m = bag_mean(st[pre + 'word_embedding.weight'], _int(title_text).reshape(n, -1), _int(title_mask).reshape(n, -1),
                 _int(content_text).reshape(n, -1), _int(content_mask).reshape(n, -1), sigmoid=True)
    c = _drop(m, keep.get('corrupt'), p)
    h = linear(c, st[pre + 'f1.weight'], st[pre + 'f1.bias'], 'sigmoid')
    d = linear(h, st[pre + 'f2.weight'], st[pre + 'f2.bias'], 'sigmoid')
    aux = row_dist(m, d, Alpha)
    cat = _drop(st[pre + 'category_embedding.weight'][_int(category).reshape(n)], keep.get('cat'), p)
    sub = _drop(st[pre + 'subCategory_embedding.weight'][_int(subCategory).reshape(n)], keep.get('sub'), p)
    return torch.cat([h, cat, sub], dim=1).view(B, N, -1), aux.view(B, N), m


def inception_call(st, title_text, title_mask, content_text, content_mask, category, subCategory, pre='news_encoder.'):
    B, N, La = np.asarray(title_text).shape if not torch.is_tensor(title_text) else title_text.shape
    n = B * N
    t, c = bag_mean(st[pre + 'word_embedding.weight'], _int(title_text).reshape(n, -1), _int(title_mask).reshape(n, -1),
                    _int(content_text).reshape(n, -1), _int(content_mask).reshape(n, -1), separate=True)
    cat = st[pre + 'category_embedding.weight'][_int(category).reshape(n)]
    sub = st[pre + 'subCategory_embedding.weight'][_int(subCategory).reshape(n)]
    e = torch.cat([t, c, cat, sub], dim=1)
    lin = lambda x, name, act: linear(x, st[pre + name + '.weight'], st[pre + name + '.bias'], act)
    s1 = lin(lin(lin(e, 'fc1_1', 'relu'), 'fc1_2', 'relu'), 'fc1_3', 'relu')
    s2 = lin(e, 'fc2', 'relu')
    s3 = t + c + cat + sub
    return lin(torch.cat([s1, s2, s3], dim=1), 'linear_transform', None).view(B, N, -1)


def att_user_rep(hist, st, pre='user_encoder.'):
    """userEncoders.py:176-191: the additive pool over ALL history slots (no mask) -> [B, D]."""
    a = torch.tanh(hist @ st[pre + 'attention.affine1.weight'].t() + st[pre + 'attention.affine1.bias']) @ st[pre + 'attention.affine2.weight'].reshape(-1)
    return torch.bmm(torch.softmax(a, dim=1).unsqueeze(1), hist).squeeze(1)


def model_forward(cfg, state, batch):
    """The whole model in float64 on a fixture's batch {field: array}: returns dict(logits, loss, aux (scalar, or None), aux_cand, cand_rep,
    hist_rep, state) with `state` the float64 leaf tensors (requires_grad) that loss.backward() fills."""
    st = {k: f64(v).requires_grad_() for k, v in state.items()}
    g = lambda k: batch[k]
    cand_in = [g('news_title_text'), g('news_title_mask'), g('news_content_text'), g('news_content_mask'), g('news_category'), g('news_subCategory')]
    hist_in = [g('user_title_text'), g('user_title_mask'), g('user_content_text'), g('user_content_mask'), g('user_category'), g('user_subCategory')]
    aux = aux_cand = None
    if cfg.news_encoder == 'DAE':
        cand, aux_c, _ = dae_call(st, *cand_in, float(cfg.Alpha))
        hist, aux_h, _ = dae_call(st, *hist_in, float(cfg.Alpha))
        aux, aux_cand = aux_h.mean(), aux_c.mean()                         # the history call's value survives
    else:
        cand, hist = inception_call(st, *cand_in), inception_call(st, *hist_in)
    if cfg.user_encoder == 'ATT':
        user = att_user_rep(hist, st).unsqueeze(1)
    else:
        pre = 'user_encoder.'
        _, user = concat_form(hist, cand, st[pre + 'affine1.weight'], st[pre + 'affine1.bias'], st[pre + 'affine2.weight'].reshape(-1),
                              st[pre + 'affine2.bias'].reshape(()), _int(g('user_history_mask')), 'relu')
    logits = (user * cand).sum(dim=2)
    loss = -(torch.log_softmax(logits, dim=1)[:, 0]).mean()
    if aux is not None:
        loss = loss + aux
    return dict(logits=logits, loss=loss, aux=aux, aux_cand=aux_cand, cand_rep=cand, hist_rep=hist, state=st)
