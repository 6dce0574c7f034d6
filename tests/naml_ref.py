"""float64 restatement of the single-view NAML news encoders NAML_Title / NAML_Content and of their multi-view attention (test
infrastructure, the oracle package does not have them), written from the formulas:

  word rows  w = keep_w / (1 - p) * word_table[text]                                         [n, L, E]
  conv       z[i, t, c] = bias[c] + sum over dt < k, e < E of W[c, e, dt] * w[i, t - (k - 1) // 2 + dt, e]   (rows outside [0, L) are zero)
             c = keep_c / (1 - p) * relu(z)                                                  [n, L, C]
  text view  t = sum_t softmax_t(a2 . tanh(A1 c + b1)) c        -- over ALL L positions, no mask: PAD positions take part
  table view a = relu(category_affine(category_table[category])),  s likewise                [n, C], no dropout
  view pool  rep = sum_v softmax_v(affine2 . tanh(affine1 F_v)) F_v  over F = (t, a, s) -- or (t0, t1, a, s) for two text views
  model      candidate call, history call, the ATT or CATT user encoder of tests/bow_ref.py, dot-product logits, -log_softmax(.)[:, 0].mean()

Everything is torch float64 with autograd on, so the backward pass is the exact derivative of these formulas.  tests/test_naml_host.py
pins it to the reference through tests/golden."""
import numpy as np
import torch

from bow_ref import f64, _int, _drop, att_user_rep
from cand_attn_ref import concat_form

STREAM = {'NAML_Title': ('title', 'max_title_length'), 'NAML_Content': ('content', 'max_abstract_length')}


def conv_rows(x, weight, bias):
    """z [n, L, C], the convolution outputs BEFORE the relu (x [n, L, E], weight [C, E, k], k odd)."""
    n, L, E = x.shape
    k = weight.shape[2]
    p = (k - 1) // 2
    xp = torch.cat([x.new_zeros(n, p, E), x, x.new_zeros(n, k - 1 - p, E)], dim=1)
    win = xp.unfold(1, k, 1)                                           # [n, L, E, k]
    return torch.einsum('nted,ced->ntc', win, weight) + bias


def additive_pool(c, w1, b1, w2):
    """layers.py:167-175 without a mask: [n, L, C] -> [n, C]."""
    a = torch.tanh(c @ w1.t() + b1) @ w2.reshape(-1)
    return torch.bmm(torch.softmax(a, dim=1).unsqueeze(1), c).squeeze(1)


def table_pre(st, pre, name, ids=None):
    """Pre-activation of a table view: affine(table) [R, C] (ids None: once per table row) or affine(table[ids]) [n, C] (per news)."""
    rows = st[pre + name + '_embedding.weight']
    if ids is not None:
        rows = rows[_int(ids).reshape(-1)]
    return rows @ st[pre + name + '_affine.weight'].t() + st[pre + name + '_affine.bias']


def view_scores(F, st, pre):
    return torch.tanh(F @ st[pre + 'affine1.weight'].t() + st[pre + 'affine1.bias']) @ st[pre + 'affine2.weight'].reshape(-1)


def view_pool(texts, scores, rowsA, scoreA, idsA, rowsB, scoreB, idsB):
    """The view pool at op level, for 1 or 2 text views: text rows [n, C] with scores [n], two table views (rows [R, C], score [R], ids [n]).
    Returns (out [n, C], alpha [n, V]) with the views in the order text views, A, B."""
    ia, ib = _int(idsA).reshape(-1), _int(idsB).reshape(-1)
    F = torch.stack(list(texts) + [rowsA[ia], rowsB[ib]], dim=1)                      # [n, V, C]
    s = torch.stack(list(scores) + [scoreA[ia], scoreB[ib]], dim=1)                   # [n, V]
    alpha = torch.softmax(s, dim=1)
    return (F * alpha.unsqueeze(2)).sum(dim=1), alpha


def naml_call(st, stream, text, category, subCategory, p=0.0, keep=None, pre='news_encoder.', per_row=False):
    """One encoder call on `text` [B, N, L] with the float64 state `st` -> (rep [B, N, C], dict(z, za, zs) of the relu pre-activations:
    convolution [n, L, C], category and subCategory affines [n, C]).  keep: {'word': [n, L, E], 'conv': [n, L, C]} keep-masks of the two
    dropout sites.  per_row: the table views evaluated once per TABLE row and indexed (what the kernels do) instead of once per news."""
    B, N, L = np.asarray(text).shape if not torch.is_tensor(text) else text.shape
    n = B * N
    keep = keep or {}
    w = _drop(st[pre + 'word_embedding.weight'][_int(text).reshape(n, L)], keep.get('word'), p)
    z = conv_rows(w, st[pre + stream + '_conv.conv.weight'], st[pre + stream + '_conv.conv.bias'])
    c = _drop(torch.relu(z), keep.get('conv'), p)
    att = pre + stream + '_attention.'
    t = additive_pool(c, st[att + 'affine1.weight'], st[att + 'affine1.bias'], st[att + 'affine2.weight'])
    ia, ib = _int(category).reshape(n), _int(subCategory).reshape(n)
    if per_row:
        rowsA, rowsB = torch.relu(table_pre(st, pre, 'category')), torch.relu(table_pre(st, pre, 'subCategory'))
        rep, _ = view_pool([t], [view_scores(t, st, pre)], rowsA, view_scores(rowsA, st, pre), ia, rowsB, view_scores(rowsB, st, pre), ib)
        za, zs = table_pre(st, pre, 'category', ia), table_pre(st, pre, 'subCategory', ib)
    else:
        za, zs = table_pre(st, pre, 'category', ia), table_pre(st, pre, 'subCategory', ib)
        F = torch.stack([t, torch.relu(za), torch.relu(zs)], dim=1)                   # [n, 3, C]
        alpha = torch.softmax(view_scores(F, st, pre), dim=1)
        rep = (F * alpha.unsqueeze(2)).sum(dim=1)
    return rep.view(B, N, -1), dict(z=z, za=za, zs=zs)


def model_forward(cfg, state, batch, p=0.0, keeps=None, per_row=False):
    """The whole model in float64 on a fixture's batch {field: array}: dict(logits, loss, cand_rep, hist_rep, pre (the relu pre-activations of
    both calls), state) with `state` the float64 leaf tensors (requires_grad) that loss.backward() fills.  keeps: (candidate call's keep
    dict, history call's keep dict) for a dropout-on run at rate p."""
    st = {k: f64(v).requires_grad_() for k, v in state.items()}
    stream = STREAM[cfg.news_encoder][0]
    g = lambda k: batch[k]
    keeps = keeps or (None, None)
    cand, pre_c = naml_call(st, stream, g('news_%s_text' % stream), g('news_category'), g('news_subCategory'), p, keeps[0], per_row=per_row)
    hist, pre_h = naml_call(st, stream, g('user_%s_text' % stream), g('user_category'), g('user_subCategory'), p, keeps[1], per_row=per_row)
    if cfg.user_encoder == 'ATT':
        user = att_user_rep(hist, st).unsqueeze(1)
    else:
        pre = 'user_encoder.'
        _, user = concat_form(hist, cand, st[pre + 'affine1.weight'], st[pre + 'affine1.bias'], st[pre + 'affine2.weight'].reshape(-1),
                              st[pre + 'affine2.bias'].reshape(()), _int(g('user_history_mask')), 'relu')
    logits = (user * cand).sum(dim=2)
    loss = -(torch.log_softmax(logits, dim=1)[:, 0]).mean()
    return dict(logits=logits, loss=loss, cand_rep=cand, hist_rep=hist, pre=dict(cand=pre_c, hist=pre_h), state=st)


def relu_margin(pre):
    """Smallest |pre-activation| of each relu input tensor relative to that tensor's scale (max |.|): {name: ratio}."""
    return {k: float(v.detach().abs().min() / v.detach().abs().max()) for k, v in pre.items()}


def site_masks(n, L, E, C, p, seed):
    """The two keep-masks one encoder call with the per-call seed `seed` draws, as the kernels key them: the word rows at seed + 1 flat over
    the compact [n, L, E], the convolution output at seed + 2 flat over the compact [n, L, C] (tests/hip_masks.py:flat_keep)."""
    from hip_masks import flat_keep
    return dict(word=flat_keep(n * L * E, p, seed + 1).view(n, L, E).cpu(), conv=flat_keep(n * L * C, p, seed + 2).view(n, L, C).cpu())
