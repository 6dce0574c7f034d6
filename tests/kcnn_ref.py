"""float64 restatement of the KCNN news encoder (DKN; test infrastructure, the oracle package does not have it), written from the formulas:

  channels   x0 = word_table[text];  x1 = tanh(entity_table[entity] M_entity^T + b);  x2 = tanh(context_table[entity] M_context^T + b)
             -- [n, L, E] each, no dropout, no mask: PAD positions take part with row 0 of each table
  conv       z[i, t, c] = bias[c] + sum over dt < w, j < 3, e < E of W[c, e, dt, j] * x_j[i, t - p + dt, e],  p = (w - 1) // 2, rows outside
             [0, L) are zero
  pool       rep[i, c] = max over t in [0, L - w + 1) of relu(z[i, t, c])   -- the first L - w + 1 positions only
  encoder    [rep | category row | subCategory row]  (the fusion's dropout is off in the fixtures)
  model      candidate call, history call, the ATT or CATT user encoder of tests/bow_ref.py, dot-product logits, -log_softmax(.)[:, 0].mean()

Everything is torch float64 with autograd on, so the backward pass is the exact derivative of these formulas (torch.max sends the gradient to
the position of the maximum).  tests/test_kcnn_host.py pins it to the reference through tests/golden."""
import numpy as np
import torch

from bow_ref import f64, _int, att_user_rep
from cand_attn_ref import concat_form


def channels(st, text, entity, pre='news_encoder.'):
    """[n, L, 3, E] from ids [n, L]."""
    text, entity = _int(text), _int(entity)
    x0 = st[pre + 'word_embedding.weight'][text]
    x1 = torch.tanh(st[pre + 'entity_embedding.weight'][entity] @ st[pre + 'M_entity.weight'].t() + st[pre + 'M_entity.bias'])
    x2 = torch.tanh(st[pre + 'context_embedding.weight'][entity] @ st[pre + 'M_context.weight'].t() + st[pre + 'M_context.bias'])
    return torch.stack([x0, x1, x2], dim=2)


def conv_rows(x, weight, bias):
    """z [n, L, C]: the convolution outputs at the L positions of the padded image, bias added (x [n, L, 3, E], weight [C, E, w, 3])."""
    n, L, _, E = x.shape
    w = weight.shape[2]
    p = (w - 1) // 2
    xp = torch.zeros((n, L + w - 1, 3, E), dtype=x.dtype)
    xp = torch.cat([xp[:, :p], x, xp[:, p + L:]], dim=1)
    win = xp.unfold(1, w, 1)                                           # [n, L, 3, E, w]
    return torch.einsum('ntjed,cedj->ntc', win, weight) + bias


def pool(z, w):
    """relu, then the maximum over the first L - w + 1 positions: [n, C]."""
    T = z.shape[1] - w + 1
    return torch.relu(z)[:, :T].max(dim=1).values


def window_ids(text, entity, w):
    """[n, L - w + 1] int: equal numbers = windows with the same content (the (word id, entity id) pairs of their w rows, -1 for a halo row).
    Two such positions of a title have the same convolution output in any precision and send the same gradients whichever the maximum picks
    (an empty history slot is all PAD: its interior windows are one and the same)."""
    text, entity = np.asarray(text), np.asarray(entity)
    n, L = text.shape
    p, T = (w - 1) // 2, L - w + 1
    rows = np.full((n, L + w - 1, 2), -1, dtype=np.int64)
    rows[:, p:p + L, 0], rows[:, p:p + L, 1] = text, entity
    wins = np.stack([rows[:, t:t + w].reshape(n, -1) for t in range(T)], axis=1)            # [n, T, 2 w]
    _, inv = np.unique(wins.reshape(n * T, -1), axis=0, return_inverse=True)
    return inv.reshape(n, T)


def margins(z, w, text, entity):
    """Per (title, channel): (top [n, C] = the positive maximum over the first L - w + 1 relu'd positions or 0, gap [n, C] = its distance to
    the best position with OTHER window content (window_ids; inf when there is none), arg [n, C] = the lowest position of the maximum)."""
    T = z.shape[1] - w + 1
    r = torch.relu(z.detach())[:, :T]
    top, arg = r.max(dim=1)
    ids = torch.from_numpy(window_ids(np.asarray(text).reshape(z.shape[0], -1), np.asarray(entity).reshape(z.shape[0], -1), w))     # [n, T]
    same = ids.unsqueeze(2) == torch.gather(ids, 1, arg)[:, None, :]                          # [n, T, C]: position t holds the winner's window
    other = torch.where(same, torch.full_like(r, -float('inf')), r).max(dim=1).values
    return top, top - other, arg


def kcnn_call(st, title_text, title_entity, category, subCategory, pre='news_encoder.'):
    """One KCNN call on [B, N, L] ids with the float64 state `st` {name: tensor} -> (rep [B, N, D], z [n, L, C])."""
    shape = np.asarray(title_text).shape if not torch.is_tensor(title_text) else title_text.shape
    B, N, L = shape
    n = B * N
    x = channels(st, _int(title_text).reshape(n, L), _int(title_entity).reshape(n, L), pre)
    weight = st[pre + 'knowledge_cnn.conv.weight']
    z = conv_rows(x, weight, st[pre + 'knowledge_cnn.conv.bias'])
    rep = pool(z, weight.shape[2])
    cat = st[pre + 'category_embedding.weight'][_int(category).reshape(n)]
    sub = st[pre + 'subCategory_embedding.weight'][_int(subCategory).reshape(n)]
    return torch.cat([rep, cat, sub], dim=1).view(B, N, -1), z


def model_forward(cfg, state, batch):
    """The whole model in float64 on a fixture's batch {field: array}: dict(logits, loss, cand_rep, hist_rep, z_cand, z_hist, state) with
    `state` the float64 leaf tensors (requires_grad) that loss.backward() fills."""
    st = {k: f64(v).requires_grad_() for k, v in state.items()}
    g = lambda k: batch[k]
    cand, z_cand = kcnn_call(st, g('news_title_text'), g('news_title_entity'), g('news_category'), g('news_subCategory'))
    hist, z_hist = kcnn_call(st, g('user_title_text'), g('user_title_entity'), g('user_category'), g('user_subCategory'))
    if cfg.user_encoder == 'ATT':
        user = att_user_rep(hist, st).unsqueeze(1)
    else:
        pre = 'user_encoder.'
        _, user = concat_form(hist, cand, st[pre + 'affine1.weight'], st[pre + 'affine1.bias'], st[pre + 'affine2.weight'].reshape(-1),
                              st[pre + 'affine2.bias'].reshape(()), _int(g('user_history_mask')), 'relu')
    logits = (user * cand).sum(dim=2)
    loss = -(torch.log_softmax(logits, dim=1)[:, 0]).mean()
    return dict(logits=logits, loss=loss, cand_rep=cand, hist_rep=hist, z_cand=z_cand, z_hist=z_hist, state=st)


def fill_entities(batch, entity_size, seed, density=0.27, empty=0.25):
    """Write entity ids into a batch's `news_title_entity` / `user_title_entity` (nnr_amd.synth leaves them zero): a quarter of the titles
    keep none, the others get a non-zero id from [1, entity_size) on about `density` of their positions -- about a fifth overall, with
    repeats across titles when entity_size is small."""
    rng = np.random.default_rng(seed)
    for k in ('news_title_entity', 'user_title_entity'):
        a = np.asarray(batch[k])
        ids = rng.integers(1, max(2, entity_size), size=a.shape)
        on = (rng.random(a.shape) < density) & (rng.random(a.shape[:2]) >= empty)[:, :, None]
        batch[k] = np.where(on, ids, 0).astype(a.dtype)
    return batch
