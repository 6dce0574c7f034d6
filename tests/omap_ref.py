"""float64 restatement of the reference's OMAP (Hi-Fi Ark) user encoder for the OMAP tests (test infrastructure; the oracle package has no
OMAP).  `omap_form` is userEncoders.py:357-369 line by line in torch ops -- bmm, masked_fill, softmax, residual, matmul, masked_fill,
softmax over the heads, bmm, bmm, softmax, bmm -- so autograd gives the reference's gradients, masked_fill's blocked ones included;
`regularizer` is :373-374.  Pinned to the reference's own results by tests/test_omap_host.py against tests/golden/*OMAP*.npz."""
import math

import numpy as np
import torch


def f64(x):
    return torch.as_tensor(np.asarray(x)).double() if not torch.is_tensor(x) else x.detach().cpu().double()


def omap_form(hist, cand, W, mask, detach_alpha=False, unblocked=False):
    """hist [B, H, D], cand [B, N, D], W [D, K], mask [B, H] or None -> dict(alpha, Y, beta, R, gamma, out).  `detach_alpha`: no gradient
    through the self-attention weights; `unblocked`: the same forward values, but the masked scores pass the softmax's gradient on (what
    the reference's masked_fill does NOT do) -- both only serve tests that show a check is not vacuous."""
    H, D, K = hist.shape[1], hist.shape[2], W.shape[1]
    s = math.sqrt(float(D))
    a = torch.bmm(hist, hist.permute(0, 2, 1)) / s
    if mask is not None:
        dead = mask.unsqueeze(1).expand(-1, H, -1) == 0
        a = a + dead * (-1e9 - a).detach() if unblocked else a.masked_fill(dead, -1e9)
    alpha = torch.softmax(a, dim=2)
    if detach_alpha:
        alpha = alpha.detach()
    Y = hist + torch.bmm(alpha, hist)
    b = torch.matmul(Y, W) / s
    if mask is not None:
        b = b.masked_fill(mask.unsqueeze(2).expand(-1, -1, K) == 0, -1e9)
    beta = torch.softmax(b, dim=2)
    R = torch.bmm(beta.permute(0, 2, 1), Y)
    gamma = torch.softmax(torch.bmm(cand, R.permute(0, 2, 1)) / s, dim=2)
    return dict(alpha=alpha, Y=Y, beta=beta, R=R, gamma=gamma, out=torch.bmm(gamma, R))


def regularizer(W, coef):
    """coef * ||(W^T W) o (J_K - I_K)||_F"""
    K = W.shape[1]
    return coef * torch.norm(torch.mm(W.transpose(1, 0), W) * (torch.ones(K, K, dtype=W.dtype) - torch.eye(K, dtype=W.dtype)), p='fro')


def _mask(mask):
    return None if mask is None else (torch.as_tensor(np.asarray(mask)) if not torch.is_tensor(mask) else mask.cpu())


def omap_user_rep(hist, cand, mask, W):
    """OMAP's user representation from recorded encoder outputs (float64)."""
    return omap_form(f64(hist), f64(cand), f64(W), _mask(mask))['out']
