"""Float64 restatement, in plain torch, of the FIM baseline: the HDC news encoder (newsEncoders.py:244-278), the matching images and the
two Conv3d + ELU + MaxPool3d layers of the FIM user encoder (userEncoders.py:244-262) and the click head (model.py:131-132).

The pooled convolution is written out so that the argmax of every pool cell is explicit: the lowest index in the window's (depth, row,
column) scan order among equal maxima (what the reference's CPU max_pool3d does), or indices handed in from outside -- autograd then sends
each cell's gradient to exactly that position (the active-set method: a backward pass is compared on the positions the kernel chose, after
those were checked to hold values within the margin of the float64 maximum)."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def t64(x):
    return torch.as_tensor(x).to(F64)


def hdc(st, text, category, subCategory, pre='news_encoder.'):
    """text [n, L], category / subCategory [n] (int64) -> d0 [n, E, S], dL [n, 3, F, S] in the reference's layout."""
    w = lambda k: t64(st[pre + k])
    word = w('word_embedding.weight')[text].permute(0, 2, 1)
    d0 = torch.cat([w('category_embedding.weight')[category].unsqueeze(2), w('subCategory_embedding.weight')[subCategory].unsqueeze(2), word], dim=2)
    x, levels = d0, []
    for l in (1, 2, 3):
        cw = w('dilated_conv%d.weight' % l)
        z = F.conv1d(x, cw, w('dilated_conv%d.bias' % l), padding=(cw.shape[2] - 1) // 2 + l - 1, dilation=l)
        g, b = w('layer_norm%d.weight' % l), w('layer_norm%d.bias' % l)
        x = torch.relu(F.layer_norm(z, list(g.shape), g, b, 1e-5))
        levels.append(x)
    return d0, torch.stack(levels, dim=1)


def images(c0, cL, h0, hL, scalar):
    """c0 [B, N, E, S], cL [B, N, 3, F, S], h0 [B, H, E, S], hL [B, H, 3, F, S] -> [B N, 4, H, S, S] (userEncoders.py:248-255)."""
    B, N = c0.shape[:2]
    H, S = h0.shape[1], h0.shape[3]
    m0 = torch.matmul(c0.unsqueeze(2).transpose(-1, -2), h0.unsqueeze(1)) / scalar
    mL = torch.matmul(cL.unsqueeze(2).transpose(-1, -2), hL.unsqueeze(1)) / scalar
    return torch.cat([m0.unsqueeze(3), mL], dim=3).permute(0, 1, 3, 2, 4, 5).reshape(B * N, 4, H, S, S)


def windows(z, P, St):
    """[n, C, D, H, W] -> [n, C, PD, PH, PW, P^3]: the pool cells' windows in (depth, row, column) scan order."""
    w = z.unfold(2, P, St).unfold(3, P, St).unfold(4, P, St)
    return w.reshape(*w.shape[:5], P * P * P)


def lowest_argmax(win):
    m = win.max(dim=-1, keepdim=True).values
    return (win == m).to(torch.int64).argmax(dim=-1)


def conv_pool(x, weight, bias, P, St, arg=None):
    """elu(maxpool3d(conv3d(x))) with explicit argmax: -> (y [n, C, PD, PH, PW], arg [n, C, PD, PH, PW] int64, z the dense convolution).
    arg given: the value at THAT window index is taken instead of the maximum."""
    z = F.conv3d(x, weight, bias)
    win = windows(z, P, St)
    if arg is None:
        arg = lowest_argmax(win.detach())
    y = F.elu(win.gather(-1, arg.unsqueeze(-1)).squeeze(-1))
    return y, arg, z


def pool_margins(z, P, St):
    """Over all pool cells of z: (smallest gap between a cell's maximum and a competitor that is not exactly equal to it, relative to
    max |z|; cells whose maximum is attained more than once; cells)."""
    win = windows(t64(z), P, St)
    m = win.max(dim=-1, keepdim=True).values
    gap = m - win
    tied = int(((gap == 0).sum(-1) > 1).sum())
    nz = gap[gap > 0]
    return (float(nz.min()) / float(t64(z).abs().max()) if nz.numel() else float('inf')), tied, int(m.numel())


def pool_sizes(S, H, cfg):
    def one(size):
        c1 = size - cfg.conv3D_kernel_size_first + 1
        p1 = (c1 - cfg.maxpooling3D_size) // cfg.maxpooling3D_stride + 1
        c2 = p1 - cfg.conv3D_kernel_size_second + 1
        return (c2 - cfg.maxpooling3D_size) // cfg.maxpooling3D_stride + 1
    return one(H), one(S), one(S)


def model(st, batch, cfg, args=None):
    """The whole forward pass in float64.  st: {reference parameter name: tensor (leaf tensors give gradients)}; batch: {field: array};
    args: (arg_a, arg_b) from outside, or None.  Returns a dict of every intermediate the tests compare."""
    g = lambda k: torch.as_tensor(batch[k]).long()
    nt, ut = g('news_title_text'), g('user_title_text')
    B, N, L = nt.shape
    H = ut.shape[1]
    c0, cL = hdc(st, nt.reshape(B * N, L), g('news_category').reshape(-1), g('news_subCategory').reshape(-1))
    h0, hL = hdc(st, ut.reshape(B * H, L), g('user_category').reshape(-1), g('user_subCategory').reshape(-1))
    S = L + 2
    c0, cL, h0, hL = c0.view(B, N, -1, S), cL.view(B, N, 3, -1, S), h0.view(B, H, -1, S), hL.view(B, H, 3, -1, S)
    img = images(c0, cL, h0, hL, math.sqrt(float(cfg.HDC_filter_num)))
    P, St = cfg.maxpooling3D_size, cfg.maxpooling3D_stride
    w = lambda k: t64(st[k])
    y1, a1, za = conv_pool(img, w('user_encoder.conv_3D_a.weight'), w('user_encoder.conv_3D_a.bias'), P, St, None if args is None else args[0])
    y2, a2, zb = conv_pool(y1, w('user_encoder.conv_3D_b.weight'), w('user_encoder.conv_3D_b.bias'), P, St, None if args is None else args[1])
    user = y2.reshape(B, N, -1)
    logits = (user @ w('fc.weight').t() + w('fc.bias')).squeeze(2)
    loss = (-torch.log_softmax(logits, dim=1)[:, 0]).mean()
    return dict(logits=logits, loss=loss, cand_d0=c0, cand_dL=cL, hist_d0=h0, hist_dL=hL, img=img, za=za, zb=zb, y1=y1, y2=y2, a1=a1, a2=a2,
                user_rep=user)


def leaf_state(arrays):
    """{name: float64 leaf tensor requiring grad} of a fixture's / make_state's arrays."""
    return {k: t64(v).clone().requires_grad_() for k, v in arrays.items()}
