"""float64 restatement of the user-encoder ablations of variantEncoders.py (SUE_wo_GCN :342-390, SUE_wo_HCA :393-419) in plain torch on the
CPU, from the history / candidate representations to the user representation, with every gradient by autograd.  The intra-cluster stage of
SUE_wo_GCN is written both ways: through the keys K(x) + b_K as the reference has it, and in the GEMV form the kernels use
(x . (W_K^T q), csrc/sue_cluster.hip); tests/test_sue_ablation_host.py pins both to the fixtures captured from the reference's own
code.  Dropout: keep-masks are handed in (tests/hip_masks.py:flat_keep gives the kernels' own), sites as SUE's."""
import math

import torch
import torch.nn.functional as F


def f64(t):
    return (t if torch.is_tensor(t) else torch.from_numpy(t)).detach().cpu().double().clone()


def seg_softmax_pool(s, x, cidx, C):
    """torch_scatter.scatter_softmax over dim 2 + scatter_sum into C clusters: s [B, N, H], x [B, H, D], cidx int64 [B, H]
    -> alpha [B, N, H], feat [B, N, C, D]; an empty cluster's row is zero."""
    onehot = F.one_hot(cidx, C).to(s.dtype)                                              # [B, H, C]
    member = onehot.bool().unsqueeze(1)                                                   # [B, 1, H, C]
    m_c = s.unsqueeze(3).masked_fill(~member, -math.inf).amax(dim=2)                      # [B, N, C]  (-inf for an empty cluster)
    m_h = torch.gather(m_c, 2, cidx.unsqueeze(1).expand(-1, s.shape[1], -1))              # [B, N, H]  (finite: h is a member)
    e = torch.exp(s - m_h.detach())
    sum_c = torch.einsum('bnh,bhc->bnc', e, onehot)
    alpha = e / torch.gather(sum_c, 2, cidx.unsqueeze(1).expand(-1, s.shape[1], -1))
    feat = torch.einsum('bnh,bhc,bhd->bncd', alpha, onehot, x)
    return alpha, feat


def seg_pool(x, u, cidx, C, scale):
    """What nnr_sue_seg_pool_fwd computes: s_h = scale <x_h, u_n>.  x [B, H, D], u [B, N, D]."""
    return seg_softmax_pool(scale * torch.einsum('bhd,bnd->bnh', x, u), x, cidx, C)


def intra_scores(x, cand, Wk, bk, Wq, bq, form):
    """[B, N, H] scores of the intra-cluster attention.  form 'keys': bmm(K(x), Q(c)) / sqrt(A) (variantEncoders.py:377-379);
    'gemv': x . (W_K^T Q(c)) / sqrt(A), which drops the b_K . Q(c) term that is common to all h of a (user, candidate)."""
    A = Wk.shape[0]
    q = cand @ Wq.t() + bq                                                                # [B, N, A]
    if form == 'keys':
        return torch.einsum('bha,bna->bnh', x @ Wk.t() + bk, q) / math.sqrt(A)
    assert form == 'gemv'
    return torch.einsum('bhd,bnd->bnh', x, q @ Wk) / math.sqrt(A)


def _margin(z):
    """Smallest |z| relative to the rms of z: how far the relu pre-activations stay from the kink, in units of their own scale."""
    z = z.detach()
    return float(z.abs().min() / z.pow(2).mean().sqrt())


def _params(state, names, grad):
    pre = 'user_encoder.'
    return {k: f64(state[pre + k]).requires_grad_(grad) for k in names}


GCN_NAMES = ('intraCluster_K.weight', 'intraCluster_K.bias', 'intraCluster_Q.weight', 'intraCluster_Q.bias', 'clusterFeatureAffine.weight',
             'clusterFeatureAffine.bias', 'interClusterAttention.K.weight', 'interClusterAttention.Q.weight', 'interClusterAttention.Q.bias')


def sue_wo_gcn(hist, cand, cmask, cidx, state, form='gemv', keep=None, p=0.0, dout=None):
    """hist [B, H, D], cand [B, N, D], cmask [B, C] (any dtype; NOT modified: the last column is set on a copy), cidx int64 [B, H],
    state {'user_encoder.<name>': array}.  keep: bool [B, N, C, D] keep-mask of the cluster-affine dropout (p its rate).
    Returns dict(user_rep, alpha, feat, relu_margin = the smallest |relu pre-activation| over the tensor's rms) and, when dout [B, N, D] is given, the gradients d hist, d cand and grad/<name>."""
    grad = dout is not None
    w = _params(state, GCN_NAMES, grad)
    x, c = f64(hist).requires_grad_(grad), f64(cand).requires_grad_(grad)
    cidx = (cidx if torch.is_tensor(cidx) else torch.from_numpy(cidx)).cpu().long()
    mask = f64(cmask) != 0
    mask[:, -1] = True
    B, N, C = x.shape[0], c.shape[1], mask.shape[1]
    A = w['intraCluster_K.weight'].shape[0]
    s = intra_scores(x, c, w['intraCluster_K.weight'], w['intraCluster_K.bias'], w['intraCluster_Q.weight'], w['intraCluster_Q.bias'], form)
    alpha, feat = seg_softmax_pool(s, x, cidx, C)
    z = feat @ w['clusterFeatureAffine.weight'].t() + w['clusterFeatureAffine.bias']
    f2 = torch.relu(z) + feat
    if keep is not None and p > 0.0:
        f2 = f2 * (f64(keep) / (1.0 - p))
    kf = f2 @ w['interClusterAttention.K.weight'].t()                                      # [B, N, C, A]
    q = c @ w['interClusterAttention.Q.weight'].t() + w['interClusterAttention.Q.bias']    # [B, N, A]
    a = torch.einsum('bnca,bna->bnc', kf, q) / math.sqrt(A)
    al = torch.softmax(a.masked_fill(~mask.unsqueeze(1), -1e9), dim=2)
    out = torch.einsum('bnc,bncd->bnd', al, f2)
    res = dict(user_rep=out.detach(), alpha=alpha.detach(), feat=feat.detach(), relu_margin=_margin(z))
    if grad:
        (out * f64(dout)).sum().backward()
        res.update(dhist=x.grad, dcand=c.grad)
        res.update({'grad/' + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()})      # (None: not in the graph)
    return res


def sue_wo_hca(hist, graph, state, N, cfg, keep_proxy=None, keep_gcn=None, p=0.0, dout=None):
    """hist [B, H, D], graph [B, G, G], state {'user_encoder.<name>': array}; cfg: gcn_layer_num, no_gcn_residual, gcn_layer_norm.
    keep_proxy: bool [B, K, D] (rate p); keep_gcn: {layer: bool [B, G, D]} (rate p / 2, not after the last layer).
    Returns dict(user_rep [B, N, D], relu_margin) and, with dout [B, N, D], d hist and grad/<name>."""
    grad = dout is not None
    Lg, res_on, ln_on = int(cfg.gcn_layer_num), not cfg.no_gcn_residual, bool(cfg.gcn_layer_norm)
    names = ['proxy_node_embedding', 'attention.affine1.weight', 'attention.affine1.bias', 'attention.affine2.weight']
    for l in range(Lg):
        names += ['gcn.gcn_layers.%d.W.weight' % l, 'gcn.gcn_layers.%d.W.bias' % l]
        if ln_on:
            names += ['gcn.gcn_layers.%d.layer_normalization.weight' % l, 'gcn.gcn_layers.%d.layer_normalization.bias' % l]
    w = _params(state, names, grad)
    x, g = f64(hist).requires_grad_(grad), f64(graph)
    B, H, D = x.shape
    proxy = w['proxy_node_embedding'].unsqueeze(0).expand(B, -1, -1)
    if keep_proxy is not None and p > 0.0:
        proxy = proxy * (f64(keep_proxy) / (1.0 - p))
    x0 = torch.cat([x, proxy], dim=1)
    out = x0
    margin = math.inf
    for l in range(Lg):
        pre = 'gcn.gcn_layers.%d.' % l
        y = torch.bmm(g, out) @ w[pre + 'W.weight'].t() + w[pre + 'W.bias']
        if ln_on:
            y = F.layer_norm(y, (D,), w[pre + 'layer_normalization.weight'], w[pre + 'layer_normalization.bias'], 1e-5)
        margin = min(margin, _margin(y))
        y = torch.relu(y)
        if res_on:
            y = y + out
        if l + 1 < Lg and keep_gcn is not None and p > 0.0:
            y = y * (f64(keep_gcn[l]) / (1.0 - p / 2))
        out = y
    gf = (out + x0)[:, :H]
    a = torch.tanh(gf @ w['attention.affine1.weight'].t() + w['attention.affine1.bias']) @ w['attention.affine2.weight'].t()   # [B, H, 1]
    alpha = torch.softmax(a.squeeze(2), dim=1)                                            # unmasked: padded slots take part
    user = torch.einsum('bh,bhd->bd', alpha, gf).unsqueeze(1).repeat(1, N, 1)
    res = dict(user_rep=user.detach(), relu_margin=margin)
    if grad:
        (user * f64(dout)).sum().backward()
        res.update(dhist=x.grad)
        res.update({'grad/' + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()})      # (None: not in the graph)
    return res
