"""float64 restatements of NPA's personalised attention for the PNE / PUE tests (test infrastructure; the oracle package has neither
encoder).  `pers_attn` is layers.CandidateAttention (layers.py:225-232) from the two projections the HIP kernel takes, with the query
taken through an index map; `pne_title_rep` is PNE's pooling stage (newsEncoders.py:359-360) from the conv stage's output, including
the `.repeat([news_num, 1])` pairing of title rows and users; `pue_user_rep` is PUE (userEncoders.py:282-283) before the expansion over
the candidates.  tests/test_npa_host.py pins the last two to the reference through tests/golden."""
import numpy as np
import torch


def f64(x):
    return torch.as_tensor(np.asarray(x)).double() if not torch.is_tensor(x) else x.detach().cpu().double()


def _mask(mask):
    if mask is None:
        return None
    return (torch.as_tensor(np.asarray(mask)) if not torch.is_tensor(mask) else mask.detach().cpu()) != 0


def pers_attn(Qf, P, uidx, w2, feature, mask):
    """Qf [n, L, A] = feature projection, P [U, A] = query projection + bias, uidx [n] (an entry outside [0, U): no query, P = 0),
    w2 [A], feature [n, L, F], mask [n, L] or None -> (alpha [n, L], out [n, F])."""
    uidx = torch.as_tensor(np.asarray(uidx) if not torch.is_tensor(uidx) else uidx.cpu()).long()
    ok = (uidx >= 0) & (uidx < P.shape[0])
    rows = P[uidx.clamp(0, P.shape[0] - 1)] * ok.unsqueeze(1).to(P.dtype)
    a = torch.tanh(Qf + rows.unsqueeze(1)) @ w2
    m = _mask(mask)
    if m is not None:
        a = a.masked_fill(~m, -1e9)
    alpha = torch.softmax(a, dim=1)
    return alpha, torch.bmm(alpha.unsqueeze(1), feature).squeeze(1)


def _cand_attention(feature, query, mask, state, pre):
    wf, wq, bq = (f64(state[pre + k]) for k in ('feature_affine.weight', 'query_affine.weight', 'query_affine.bias'))
    w2 = f64(state[pre + 'attention_affine.weight']).reshape(-1)
    a = torch.tanh(feature @ wf.t() + (query @ wq.t() + bq).unsqueeze(1)) @ w2
    m = _mask(mask)
    if m is not None:
        a = a.masked_fill(~m, -1e9)
    alpha = torch.softmax(a, dim=1)
    return torch.bmm(alpha.unsqueeze(1), feature).squeeze(1)


def pne_title_rep(c, user_rows, state, B, news_num, mask=None, intended=False, pre='news_encoder.'):
    """c [B * news_num, L, C] = the conv stage's output (after its dropout), user_rows [B, user_embedding_dim] = the rows Model.forward
    hands to the encoder, mask [B * news_num, L] -> the pooled title representation [B * news_num, C] (before feature fusion).
    Row r attends with user r % B, as `.repeat([news_num, 1])` pairs them; intended=True pairs it with its owner r // news_num instead."""
    c, user_rows = f64(c), f64(user_rows)
    q = torch.relu(user_rows @ f64(state[pre + 'dense.weight']).t() + f64(state[pre + 'dense.bias']))
    r = torch.arange(B * news_num)
    q_w = q[r // news_num] if intended else q[r % B]
    return _cand_attention(c.reshape(B * news_num, c.shape[-2], c.shape[-1]), q_w, mask, state, pre + 'personalizedAttention.')


def pue_user_rep(hist_rep, user_rows, mask, state, pre='user_encoder.'):
    """hist_rep [B, H, D], user_rows [B, user_embedding_dim], mask [B, H] -> the user representation [B, D] (before `.expand`)."""
    q_d = torch.relu(f64(user_rows) @ f64(state[pre + 'dense.weight']).t() + f64(state[pre + 'dense.bias']))
    return _cand_attention(f64(hist_rep), q_d, mask, state, pre + 'personalizedAttention.')
