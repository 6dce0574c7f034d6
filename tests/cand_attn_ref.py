"""float64 restatement of the reference's candidate-aware additive attention for the CATT / CandidateAttention tests (test
infrastructure; the oracle package has no CATT).  `concat_form` is the reference's own formulation -- expand, concat, Linear,
activation, Linear, masked_fill, softmax, weighted sum (userEncoders.py:213-220; layers.py:225-232, 254-262 are the same with the
Linear split in two) -- and is pinned to the reference by tests/test_catt_host.py against tests/golden; `pq_form` is the same
arithmetic from the two projections the HIP kernel takes, pinned to `concat_form` there too."""
import numpy as np
import torch

ACTS = {'relu': torch.relu, 'tanh': torch.tanh}


def concat_form(feat, query, W1, b1, w2, b2, mask, act):
    """feat [B, H, F], query [B, N, Qd], W1 [A, Qd + F] (on [query ; feat]), b1 [A], w2 [A], b2 scalar, mask [B, H] or None -> (alpha, out)"""
    H, N = feat.shape[1], query.shape[1]
    cat = torch.cat([query.unsqueeze(2).expand(-1, -1, H, -1), feat.unsqueeze(1).expand(-1, N, -1, -1)], dim=3)
    a = ACTS[act](cat @ W1.t() + b1) @ w2 + b2
    if mask is not None:
        a = a.masked_fill(mask.unsqueeze(1).expand(-1, N, -1) == 0, -1e9)
    alpha = torch.softmax(a, dim=2)
    return alpha, torch.bmm(alpha, feat)


def pq_form(P, Q, w2, feat, mask, act):
    """P [B, N, A] = query projection + bias, Q [B, H, A] = feature projection -> (alpha, out)"""
    a = ACTS[act](P.unsqueeze(2) + Q.unsqueeze(1)) @ w2
    if mask is not None:
        a = a.masked_fill(mask.unsqueeze(1).expand(-1, P.shape[1], -1) == 0, -1e9)
    alpha = torch.softmax(a, dim=2)
    return alpha, torch.bmm(alpha, feat)


def f64(x):
    return torch.as_tensor(np.asarray(x)).double() if not torch.is_tensor(x) else x.detach().cpu().double()


def catt_user_rep(hist, cand, mask, state, pre='user_encoder.'):
    """CATT's user representation from recorded encoder outputs and a {name: array} state (float64)."""
    alpha, out = concat_form(f64(hist), f64(cand), f64(state[pre + 'affine1.weight']), f64(state[pre + 'affine1.bias']),
                             f64(state[pre + 'affine2.weight']).reshape(-1), f64(state[pre + 'affine2.bias']).reshape(()),
                             torch.as_tensor(np.asarray(mask)) if not torch.is_tensor(mask) else mask.cpu(), 'relu')
    return out
