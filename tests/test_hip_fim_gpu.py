"""GPU tests of the FIM baseline: the kernels of csrc/fim.hip and csrc/hdc.hip op by op against tests/fim_ref.py in float64, and the model
against the reference's own results (tests/golden/*HDC_FIM*.npz) on both matrix paths.

Pooled convolution, the active-set method: the forward argmax is checked first -- every index the kernel chose must hold a value within M
of the float64 maximum of its cell, M = 20 x the deviation of torch's own fp32 convolution from float64 on the same data, relative to the
largest absolute convolution output --, then the float64 backward pass runs WITH the kernel's indices and must agree."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fim_ref
from fim_ref import t64
from golden_io import GoldenCase, build_model, eval_fixture
from test_fim_host import restated, fixture_margin, TINY, FULL

pytestmark = pytest.mark.gpu

OP_BAR = 1e-5              # op level: of each tensor's own scale
BAR = 1e-4                 # model level, the project's bar
MARGIN_FACTOR = 20.0
DENSE_A_BYTES = 10 * 32 * 48 * 32 * 32 * 4


def dev():
    return torch.device('cuda')


def _close(name, got, exp, bar, scale=None):
    exp = t64(exp)
    got = t64(got.detach().cpu()).reshape(exp.shape)
    s = float(exp.abs().max()) if scale is None else scale
    err = float((got - exp).abs().max())
    print('%s: max |err| %.2e of scale %.2e (bar %.0e)' % (name, err, s, bar))
    assert err <= bar * s, (name, err, s)


# ------------------------------------------------------------------------------------------------ fused Conv3d + ELU + MaxPool3d
CONV_CASES = {
    'one_cell': dict(imgs=2, Cin=4, dims=(5, 5, 5), Cout=8, K=3, P=3, St=3),
    'remainders': dict(imgs=2, Cin=4, dims=(9, 10, 12), Cout=8, K=3, P=3, St=3),
    'layer_b': dict(imgs=3, Cin=32, dims=(16, 10, 10), Cout=16, K=3, P=3, St=3, channel_last=True, cf=True),
    'channels_3_5': dict(imgs=2, Cin=3, dims=(7, 8, 9), Cout=5, K=3, P=2, St=2, channel_last=True),
    'kernel_2': dict(imgs=2, Cin=4, dims=(6, 7, 8), Cout=6, K=2, P=3, St=3),
    'kernel_4_1': dict(imgs=1, Cin=2, dims=(7, 7, 9), Cout=4, K=4, P=1, St=1),
    'pool_2_2': dict(imgs=2, Cin=4, dims=(11, 12, 12), Cout=3, K=3, P=2, St=2),
    'pool_2_stride_3': dict(imgs=2, Cin=4, dims=(10, 11, 12), Cout=4, K=3, P=2, St=3),
    'one_image': dict(imgs=1, Cin=4, dims=(9, 12, 12), Cout=8, K=3, P=3, St=3),
    'seven_images': dict(imgs=7, Cin=4, dims=(8, 8, 8), Cout=8, K=3, P=3, St=3, cf=True),
    'many_rows': dict(imgs=2, Cin=4, dims=(5, 34, 34), Cout=32, K=3, P=3, St=3),
    # one pool cell per image: the weight gradient sums one partial row per image -- 1, 4 and 5 rows, around its groups of four loads
    'one_partial_row': dict(imgs=1, Cin=4, dims=(5, 5, 5), Cout=8, K=3, P=3, St=3),
    'four_partial_rows': dict(imgs=4, Cin=4, dims=(5, 5, 5), Cout=8, K=3, P=3, St=3),
    'five_partial_rows': dict(imgs=5, Cin=3, dims=(5, 5, 5), Cout=5, K=3, P=3, St=3),
}


def _conv_inputs(c, constant=False):
    g = torch.Generator().manual_seed(101 + c['Cin'] * 7 + c['Cout'])
    D, H, W = c['dims']
    x = torch.randn(c['imgs'], c['Cin'], D, H, W, generator=g)
    if constant:
        x = torch.full_like(x, 0.37)
    w = torch.randn(c['Cout'], c['Cin'], c['K'], c['K'], c['K'], generator=g) / (c['Cin'] * c['K'] ** 3) ** 0.5
    b = 0.1 * torch.randn(c['Cout'], generator=g)
    return x, w, b


def _run_conv(c, x, w, b, dy=None):
    """The kernel pair on x [imgs, Cin, D, H, W] (laid out channel-last on the device when the case says so).  Returns y, arg as
    [imgs, Cout, PD, PH, PW] and, with dy [imgs, Cout, PD, PH, PW], (dx [imgs, Cin, D, H, W], dw, db)."""
    from nnr_amd import ops
    d = dev()
    imgs, Cin, Cout, K, P, St = c['imgs'], c['Cin'], c['Cout'], c['K'], c['P'], c['St']
    D, H, W = c['dims']
    cl, cf = c.get('channel_last', False), c.get('cf', False)
    PD, PH, PW = ops.conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St)
    cells = PD * PH * PW
    if cl:
        xd = x.permute(0, 2, 3, 4, 1).contiguous().to(d)
        strides = (D * H * W * Cin, 1, H * W * Cin, W * Cin, Cin)
    else:
        xd = x.contiguous().to(d)
        strides = (Cin * D * H * W, D * H * W, H * W, W, 1)
    wd, bd = w.to(d), b.to(d)
    y = torch.full((imgs, cells * Cout), float('nan'), device=d)
    arg = torch.full((imgs, cells * Cout), 255, device=d, dtype=torch.uint8)
    ops.conv3d_pool_fwd(xd, strides, ops.conv3d_weight(wd, 0), bd, imgs, Cin, D, H, W, Cout, K, P, St, cf, y, arg)
    unpack = (lambda t: t.view(imgs, Cout, PD, PH, PW)) if cf else (lambda t: t.view(imgs, PD, PH, PW, Cout).permute(0, 4, 1, 2, 3))
    out = [unpack(y).cpu(), unpack(arg).cpu().long()]
    if dy is not None:
        dyd = (dy if cf else dy.permute(0, 2, 3, 4, 1)).contiguous().to(d)
        runs = []
        for _ in range(2):
            dx = torch.full_like(xd, float('nan'))
            dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
            ops.conv3d_pool_bwd(dyd, y, arg, xd, strides, ops.conv3d_weight(wd, 1), imgs, Cin, D, H, W, Cout, K, P, St, cf, dx, dw, db)
            torch.cuda.synchronize()
            runs.append((dx.cpu(), dw.cpu(), db.cpu()))
        for a, e in zip(*runs):
            assert torch.equal(a, e), 'two backward runs differ'
        dx = runs[0][0]
        out.append((dx.permute(0, 4, 1, 2, 3) if cl else dx, runs[0][1], runs[0][2]))
    return out


@pytest.mark.parametrize('name', list(CONV_CASES))
def test_conv3d_pool_forward_argmax_and_backward(name):
    c = CONV_CASES[name]
    x, w, b = _conv_inputs(c)
    P, St = c['P'], c['St']
    x64, w64, b64 = (t64(t).requires_grad_() for t in (x, w, b))
    y_ref, a_ref, z = fim_ref.conv_pool(x64, w64, b64, P, St)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(y_ref.shape, generator=g)
    y, arg, (dx, dw, db) = _run_conv(c, x, w, b, dy)
    assert y.shape == y_ref.shape
    _close(name + ' y', y, y_ref.detach(), OP_BAR)
    # the argmax first: within M of the float64 maximum
    zs = float(z.detach().abs().max())
    M = MARGIN_FACTOR * float((F.conv3d(x, w, b).double() - z.detach()).abs().max()) / zs
    win = fim_ref.windows(z.detach(), P, St)
    assert int(arg.max()) < P ** 3
    gap = (win.max(dim=-1).values - win.gather(-1, arg.unsqueeze(-1)).squeeze(-1)) / zs
    print('%s: M %.2e, largest gap of a chosen index %.2e, indices that differ from float64 %d of %d' %
          (name, M, float(gap.max()), int((arg != a_ref).sum()), arg.numel()))
    assert float(gap.max()) <= M
    # then the float64 backward pass with the kernel's indices
    y_act = fim_ref.conv_pool(x64, w64, b64, P, St, arg=arg)[0]
    (y_act * t64(dy)).sum().backward()
    _close(name + ' dx', dx, x64.grad, OP_BAR)
    _close(name + ' dw', dw, w64.grad, OP_BAR)
    _close(name + ' db', db, b64.grad, OP_BAR)


def test_host_shape_rules_mirror_the_library():
    """ops.conv3d_pool_plan (what Model.__init__ checks without a device) against nnr_conv3d_pool_dims over a sweep that crosses every limit,
    the LDS one included."""
    from nnr_amd import ops, _lib
    n_ok = n_bad = 0
    for Cin, Cout in ((4, 32), (32, 16), (3, 5), (64, 64), (200, 40), (4, 700)):
        for D, H, W in ((50, 34, 34), (16, 10, 10), (5, 5, 5), (9, 10, 300), (4, 9, 9), (12, 12, 12)):
            for K, P, St in ((3, 3, 3), (3, 2, 2), (2, 3, 3), (4, 1, 1), (3, 2, 3), (3, 3, 2), (5, 3, 3), (3, 5, 5), (4, 4, 4)):
                want = ops.conv3d_pool_plan(Cin, D, H, W, Cout, K, P, St)
                try:
                    got = ops.conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St)
                except _lib.NnrHipError:
                    got = None
                assert got == want, (Cin, Cout, D, H, W, K, P, St, got, want)
                n_ok, n_bad = n_ok + (got is not None), n_bad + (got is None)
    assert n_ok > 50 and n_bad > 50
    assert ops.conv3d_pool_plan(4, 9, 10, 300, 700, 3, 3, 3) is None and ops.conv3d_pool_plan(200, 12, 12, 12, 40, 4, 4, 4) is None      # the LDS limit alone


def test_conv3d_pool_constant_image_ties_go_to_index_zero():
    c = dict(imgs=2, Cin=4, dims=(8, 8, 9), Cout=8, K=3, P=3, St=3)
    x, w, b = _conv_inputs(c, constant=True)
    dy = torch.ones(2, 8, 2, 2, 2)
    y, arg, (dx, dw, db) = _run_conv(c, x, w, b, dy)
    assert int(arg.abs().max()) == 0, 'a tie must go to the lowest index'
    first = torch.zeros(8, 8, 9, dtype=torch.bool)
    for pd in range(2):
        for ph in range(2):
            for pw in range(2):
                first[pd * 3:pd * 3 + 3, ph * 3:ph * 3 + 3, pw * 3:pw * 3 + 3] = True
    assert bool((dx[:, :, ~first] == 0).all()) and bool((dx[:, :, first].abs().sum() > 0))
    x64, w64, b64 = (t64(t).requires_grad_() for t in (x, w, b))
    (fim_ref.conv_pool(x64, w64, b64, 3, 3)[0] * t64(dy)).sum().backward()
    _close('constant dx', dx, x64.grad, OP_BAR)


@pytest.mark.parametrize('over', [dict(P=3, St=2), dict(K=5), dict(P=5, St=5, dims=(12, 12, 12)), dict(dims=(4, 9, 9)), dict(dims=(9, 9, 3))],
                         ids=['overlap', 'kernel5', 'pool5', 'no_cell_depth', 'no_cell_column'])
def test_conv3d_pool_refuses_unsupported_shapes(over):
    from nnr_amd import ops, _lib
    c = dict(imgs=1, Cin=2, dims=(9, 9, 9), Cout=4, K=3, P=3, St=3)
    c.update(over)
    d = dev()
    D, H, W = c['dims']
    K = c['K']
    x = torch.randn(1, 2, D, H, W, device=d)
    wp = torch.randn(2 * K ** 3 * 4, device=d)
    y = torch.full((64,), float('nan'), device=d)
    arg = torch.full((64,), 77, device=d, dtype=torch.uint8)
    strides = (2 * D * H * W, D * H * W, H * W, W, 1)
    with pytest.raises(_lib.NnrHipError, match='unsupported size'):
        ops.conv3d_pool_dims(2, D, H, W, 4, K, c['P'], c['St'])
    rc = _lib.lib().nnr_conv3d_pool_fwd(x.data_ptr(), *strides, wp.data_ptr(), wp.data_ptr(), 1, 2, D, H, W, 4, K, c['P'], c['St'], 0, y.data_ptr(),
                                        arg.data_ptr(), ops._s())
    assert rc == -3
    dx = torch.full_like(x, float('nan'))
    dw = torch.full((4 * 2 * K ** 3,), float('nan'), device=d)
    rc = _lib.lib().nnr_conv3d_pool_bwd(y.data_ptr(), y.data_ptr(), arg.data_ptr(), x.data_ptr(), *strides, wp.data_ptr(), 1, 2, D, H, W, 4, K, c['P'],
                                        c['St'], 0, dx.data_ptr(), dw.data_ptr(), dw.data_ptr(), dw.data_ptr(), ops._s())
    assert rc == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool((arg == 77).all()) and bool(torch.isnan(dx).all()) and bool(torch.isnan(dw).all())


# ------------------------------------------------------------------------------------------------ matching images
def test_matching_images_forward_and_backward():
    from nnr_amd import ops
    B, N, H, S = 2, 3, 4, 7
    g = torch.Generator().manual_seed(9)
    d = dev()
    alpha = 1.0 / 10 ** 0.5
    c0, h0 = torch.randn(B * N, S, 6, generator=g), torch.randn(B * H, S, 6, generator=g)
    cL, hL = torch.randn(3, B * N, S, 10, generator=g), torch.randn(3, B * H, S, 10, generator=g)
    levels = [(c0, h0)] + [(cL[l], hL[l]) for l in range(3)]
    plane = B * N * S * H * S
    img = torch.full((4, plane), float('nan'), device=d)
    for l, (c, h) in enumerate(levels):
        ops.match_images_fwd(c.to(d), h.to(d), B, N, H, S, alpha, img[l])
    # the reference's layout and formula: [B, N, E, S] / [B, N, 3, F, S] operands
    r = lambda t, n: t64(t).view(B, n, S, -1).transpose(2, 3)
    ref = fim_ref.images(r(c0, N), torch.stack([r(cL[l], N) for l in range(3)], dim=2), r(h0, H), torch.stack([r(hL[l], H) for l in range(3)], dim=2),
                         10 ** 0.5)                                      # [B N, 4, H, S, S]
    got = img.cpu().view(4, B * N, S, H, S).permute(1, 0, 3, 2, 4)
    _close('images', got, ref, OP_BAR)
    dimg = torch.randn(4, plane, generator=g)
    for l, (c, h) in enumerate(levels):
        c64, h64 = t64(c).requires_grad_(), t64(h).requires_grad_()
        im = alpha * torch.matmul(c64.view(B, N * S, -1), h64.view(B, H * S, -1).transpose(1, 2))
        (im * t64(dimg[l]).view(B, N * S, H * S)).sum().backward()
        runs = []
        for _ in range(2):
            dc, dh = torch.full_like(c, float('nan'), device=d), torch.full_like(h, float('nan'), device=d)
            ops.match_images_bwd(dimg[l].to(d), c.to(d), h.to(d), B, N, H, S, alpha, dc, dh)
            runs.append((dc.cpu(), dh.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        _close('level %d dcand' % l, runs[0][0], c64.grad, OP_BAR)
        _close('level %d dhist' % l, runs[0][1], h64.grad, OP_BAR)


# ------------------------------------------------------------------------------------------------ LayerNorm([F, S]) + ReLU
@pytest.mark.parametrize('FS', [(6, 7), (150, 34)], ids=['6x7', '150x34'])
def test_layernorm_relu_forward_and_backward(FS):
    """Three news; news 1 has a constant input, so its pre-activation is beta, negative everywhere: output and input gradient zero.  The
    rows behind a news' S live rows hold NaN going in and zero coming out of the backward call."""
    _layernorm_relu_case(FS[0], FS[1], 3)


@pytest.mark.parametrize('n', [100, 130])
def test_layernorm_relu_backward_over_several_chunks_of_news(n):
    """The affine gradients are summed from one partial row per 32 news: 4 and 5 rows (the three news of the test above: one)."""
    _layernorm_relu_case(6, 7, n)


def _layernorm_relu_case(Fn, S, n):
    from nnr_amd import ops
    pad, d = 2, dev()
    Sp = S + 2 * pad
    g = torch.Generator().manual_seed(13 + Fn)
    z = torch.full((n, Sp, Fn), float('nan'))
    z[:, :S] = 2.0 * torch.randn(n, S, Fn, generator=g) + 0.5
    z[1, :S] = 1.25
    gamma, beta = 1.0 + 0.5 * torch.randn(Fn, S, generator=g), -0.25 - 0.1 * torch.rand(Fn, S, generator=g)
    dy = torch.randn(n, S, Fn, generator=g)
    zd, gd, bd = z.to(d), gamma.to(d), beta.to(d)
    y = torch.full((n, S, Fn), float('nan'), device=d)
    yp = torch.full((n, S + 6, Fn), float('nan'), device=d)
    stats = torch.empty((n, 2), device=d)
    ops.hdc_ln_relu_fwd(zd.view(n * Sp, Fn), Sp, gd, bd, n, S, Fn, 1e-5, y, yp, 3, stats)
    z64, g64, b64 = t64(z[:, :S]).requires_grad_(), t64(gamma).requires_grad_(), t64(beta).requires_grad_()
    ref = torch.relu(F.layer_norm(z64.transpose(1, 2), [Fn, S], g64, b64, 1e-5)).transpose(1, 2)        # [n, S, F]
    _close('ln y', y, ref.detach(), OP_BAR)
    assert torch.equal(yp[:, 3:3 + S], y) and bool((yp[:, :3] == 0).all()) and bool((yp[:, 3 + S:] == 0).all())
    assert bool((y[1] == 0).all()) and float(ref[1].detach().abs().max()) == 0.0
    (ref * t64(dy)).sum().backward()
    runs = []
    for _ in range(2):
        zz = zd.clone()
        dg, db = torch.zeros_like(gd), torch.zeros_like(bd)
        ops.hdc_ln_relu_bwd(dy.to(d), y, zz.view(n * Sp, Fn), Sp, stats, gd, n, S, Fn, dg, db)
        runs.append((zz.cpu(), dg.cpu(), db.cpu()))
    for a, e in zip(*runs):
        assert torch.equal(a, e)
    dz, dg, db = runs[0]
    assert bool((dz[:, S:] == 0).all()) and bool((dz[1] == 0).all())
    _close('ln dz', dz[:, :S], z64.grad, OP_BAR)
    _close('ln dgamma', dg, g64.grad, OP_BAR)
    _close('ln dbeta', db, b64.grad, OP_BAR)


# ------------------------------------------------------------------------------------------------ sequence image
def test_sequence_image_and_its_table_gradients():
    from nnr_amd import ops
    n, L, E, pad, V, ncat, nsub = 5, 6, 10, 1, 9, 3, 4
    S, d = L + 2, dev()
    g = torch.Generator().manual_seed(17)
    word, cat_t, sub_t = torch.randn(V, E, generator=g), torch.randn(ncat, E, generator=g), torch.randn(nsub, E, generator=g)
    text = torch.randint(1, V, (n, L), generator=g, dtype=torch.int32)
    text[:, 4:] = 0                                                   # PAD positions read row 0, which takes gradient
    text[1] = text[0]                                                 # repeated words
    cat, sub = torch.tensor([0, 2, 2, 1, 0], dtype=torch.int32), torch.tensor([3, 3, 0, 1, 3], dtype=torch.int32)
    d0 = torch.full((n, S, E), float('nan'), device=d)
    d0p = torch.full((n, S + 2 * pad, E), float('nan'), device=d)
    toks = torch.full((3, n * S), -7, device=d, dtype=torch.int32)
    ops.hdc_seq_fwd(word.to(d), cat_t.to(d), sub_t.to(d), text.reshape(-1).to(d), cat.to(d), sub.to(d), n, L, pad, d0, d0p, toks[0], toks[1], toks[2])
    exp = torch.cat([cat_t[cat.long()].unsqueeze(1), sub_t[sub.long()].unsqueeze(1), word[text.long()]], dim=1)
    assert torch.equal(d0.cpu(), exp) and torch.equal(d0p[:, pad:pad + S].cpu(), exp)
    assert bool((d0p[:, :pad] == 0).all()) and bool((d0p[:, pad + S:] == 0).all())
    tk = toks.cpu().view(3, n, S)
    assert torch.equal(tk[0][:, 2:], text) and bool((tk[0][:, :2] == -1).all())
    assert torch.equal(tk[1][:, 0], cat) and bool((tk[1][:, 1:] == -1).all()) and torch.equal(tk[2][:, 1], sub) and bool((tk[2][:, [0] + list(range(2, S))] == -1).all())
    dx = torch.randn(n * S, E, generator=g)
    ref = [torch.zeros(V, E, dtype=torch.float64), torch.zeros(ncat, E, dtype=torch.float64), torch.zeros(nsub, E, dtype=torch.float64)]
    dx64 = t64(dx).view(n, S, E)
    ref[0].index_add_(0, text.long().reshape(-1), dx64[:, 2:].reshape(-1, E))
    ref[1].index_add_(0, cat.long(), dx64[:, 0])
    ref[2].index_add_(0, sub.long(), dx64[:, 1])
    runs = []
    for _ in range(2):
        grads = [torch.zeros(V, E, device=d), torch.zeros(ncat, E, device=d), torch.zeros(nsub, E, device=d)]
        for j, gt in enumerate(grads):
            ts = ops.TokenSort(toks[j], None, gt.shape[0])
            ops.embed_scatter_sorted(dx.to(d), ts, gt, 0.0, 0)
        ops.join_extra_streams()
        torch.cuda.synchronize()
        runs.append([gt.cpu() for gt in grads])
    for a, e, r in zip(runs[0], runs[1], ref):
        assert torch.equal(a, e)
        _close('table gradient', a, r, OP_BAR)


# ------------------------------------------------------------------------------------------------ the model
ZERO_ON_PAPER = {'fc.bias': 'fc.weight'}      # the softmax loss does not see a shift common to all candidates: 0 on paper
CANCELLING = ('user_encoder.conv_3D_a.bias', 'user_encoder.conv_3D_b.bias')
ZERO_GRADIENT = ('fc.bias', 'user_encoder.conv_3D_b.bias')     # tensors with an element whose gradient is zero on paper


def _position_major(rep):
    """(d0 [B, N, S, E], dL [3, B, N, S, F]) -> the reference's ([B, N, E, S], [B, N, 3, F, S])."""
    d0, dL = rep
    return d0.detach().cpu().permute(0, 1, 3, 2), dL.detach().cpu().permute(1, 2, 0, 4, 3)


@pytest.mark.parametrize('bx3', [True, False], ids=['bx3', 'f32_mfma'])
@pytest.mark.parametrize('tag', TINY)
def test_model_matches_reference_golden(tag, bx3):
    """Logits, loss, both representation pairs and every parameter gradient within 1e-4 of each tensor's scale, against the reference's
    float64 run; the kernel's argmax indices within the fixture's margin M; parameters after Adam steps 1 and 3 against the fixture."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    from nnr_amd.trainer import Trainer
    case = GoldenCase(tag)
    before = ops.BX3[0]
    ops.BX3[0] = bx3
    try:
        model, cfg = build_model(case, 'train')
        trainer = Trainer(model, cfg)
        reps = []
        model.news_encoder.register_forward_hook(lambda m, i, o: reps.append(_position_major(o)))
        steps = int(case.meta['adam_steps'])
        for s in range(steps):
            trainer.flat.zero_grad()
            logits = model(*case.batch('cuda'))
            loss = negative_log_softmax(logits)
            loss.backward()
            ops.join_extra_streams()
            torch.cuda.synchronize()
            if s == 0:
                _close('logits', logits, case.expect('f64/logits'), BAR)
                _close('loss', loss, case.expect('f64/loss'), BAR)
                for key, rep in (('cand_rep', reps[0]), ('hist_rep', reps[1])):
                    _close(key + '/d0', rep[0], case.expect('f64/%s/d0' % key), BAR)
                    _close(key + '/dL', rep[1], case.expect('f64/%s/dL' % key), BAR)
                scale = {k: float(np.abs(case.expect('f64/grad/' + k)).max()) for k, _ in model.named_parameters() if not k.startswith('user_encoder.news_encoder.')}
                for k, p in model.named_parameters():
                    if k not in scale:
                        continue
                    bar = BAR
                    if k in CANCELLING:      # cancellation: the reference's own fp32 gradient sits this far from float64
                        own = float(np.abs(case.expect('grad/' + k).astype(np.float64) - case.expect('f64/grad/' + k)).max()) / scale[k]
                        bar = max(BAR, 4.0 * own)
                        print('%s: the fixture\'s own fp32 distance %.2e -> bar %.2e' % (k, own, bar))
                    _close('grad ' + k, p.grad, case.expect('f64/grad/' + k), bar, scale=scale[ZERO_ON_PAPER.get(k, k)])
            assert abs(float(loss) - float(case.expect('loss_step%d' % s))) <= 5e-5 * max(1.0, abs(float(case.expect('loss_step%d' % s)))), 'loss at step %d' % s
            trainer.optimizer_step(1.0)
            if s in (0, steps - 1):
                torch.cuda.synchronize()
                lr = float(cfg.lr)
                for k, p in model.named_parameters():
                    if k.startswith('user_encoder.news_encoder.'):
                        continue
                    exp, act = case.expect_param(s + 1, k, p)
                    dlt = np.abs(act - exp)
                    # Adam moves an element by at most lr per step whatever its gradient, in the direction of its sign: the project's bound.
                    # Where the gradient is zero on paper (ZERO_GRADIENT: fc.bias; conv_3D_b.bias[0], 1.7e-16 in the reference's float64 run and
                    # -1.5e-7 in its fp32 run) that sign is rounding noise in any implementation, so two runs can part by 2 lr per step
                    per_step = 2 if k in ZERO_GRADIENT else 1
                    assert dlt.max(initial=0.0) <= per_step * (s + 1) * lr * 1.01 + 1e-4, 'param (hard bound) %s after step %d' % (k, s + 1)
                    if float(case.expect('gradnorm/' + k)) >= 1e-2 * float(case.expect('grad_total_norm')):
                        assert float(dlt.mean()) <= max(2e-5, 0.05 * (s + 1) * lr), 'param (mean deviation) %s after step %d' % (k, s + 1)
    finally:
        ops.BX3[0] = before


@pytest.mark.parametrize('tag', TINY)
def test_model_argmax_is_within_the_fixture_margin(tag):
    """The user encoder on the reference's float64 representations (rounded to fp32): every index of both layers points at a value within
    M of the float64 maximum.  One matrix path suffices: ops.BX3 moves weight-operand NT products onto the bf16 pipe, and the user encoder runs none
    (its products are activation against activation; the rest is csrc/fim.hip)."""
    from nnr_amd import ops
    case, st, out = restated(tag)
    M, _ = fixture_margin(case)
    model, cfg = build_model(case, 'train')
    ue = model.user_encoder
    pm = lambda d0, dL: (d0.detach().permute(0, 1, 3, 2).float().contiguous().cuda(), dL.detach().permute(2, 0, 1, 4, 3).float().contiguous().cuda())
    cand, hist = pm(out['cand_d0'], out['cand_dL']), pm(out['hist_d0'], out['hist_dL'])
    caught = {}
    orig = ops.conv3d_pool_fwd

    def spy(x, strides, wp, bias, imgs, Cin, D, H, W, Cout, K, P, St, cf, y, arg):
        orig(x, strides, wp, bias, imgs, Cin, D, H, W, Cout, K, P, St, cf, y, arg)
        PD, PH, PW = ops.conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St)
        caught['b' if cf else 'a'] = (arg.view(imgs, Cout, PD, PH, PW) if cf else arg.view(imgs, PD, PH, PW, Cout).permute(0, 4, 1, 2, 3)).cpu().long()
    ops.conv3d_pool_fwd = spy
    try:
        user = ue.encode_user(hist, None, None, None, None, cand)
    finally:
        ops.conv3d_pool_fwd = orig
    P, St = cfg.maxpooling3D_size, cfg.maxpooling3D_stride
    for key, zname in (('a', 'za'), ('b', 'zb')):
        z = out[zname].detach()
        win = fim_ref.windows(z, P, St)
        gap = (win.max(dim=-1).values - win.gather(-1, caught[key].unsqueeze(-1)).squeeze(-1)) / float(z.abs().max())
        print('%s layer %s: M %.2e, largest gap of a chosen index %.2e' % (tag, key, M, float(gap.max())))
        assert float(gap.max()) <= M
    _close('user_rep', user, out['user_rep'].detach(), BAR)


@pytest.mark.parametrize('bx3', [True, False], ids=['bx3', 'f32_mfma'])
def test_model_at_the_default_shapes(bx3):
    """The full-size fixture (batch 2) on both matrix paths: logits and loss against the reference's fp32 run, every stored gradient element
    within 1e-4 of the tensor's float64 scale (tests/fim_ref.py on the same weights and batch)."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    case, st, out = restated(FULL)
    before = ops.BX3[0]
    ops.BX3[0] = bx3
    try:
        model, cfg = build_model(case, 'train')
        logits = model(*case.batch('cuda'))
        loss = negative_log_softmax(logits)
        loss.backward()
        ops.join_extra_streams()
        torch.cuda.synchronize()
    finally:
        ops.BX3[0] = before
    _close('logits', logits, case.expect('logits'), BAR)
    _close('loss', loss, case.expect('loss'), BAR)
    for k, p in model.named_parameters():
        if k.startswith('user_encoder.news_encoder.'):
            continue
        exp, act = case.expect_grad(k, p.grad)
        s = float(st[ZERO_ON_PAPER.get(k, k)].grad.abs().max())
        err = float(np.abs(act.astype(np.float64) - exp).max())
        print('grad %s: %.2e of scale %.2e' % (k, err, s))
        assert err <= BAR * s, (k, err, s)


def test_user_encoder_never_holds_a_dense_convolution_output():
    """encode_user forward + backward at the default shapes, batch 2: the peak extra device allocation stays below ONE dense first-layer
    convolution output (10 x 32 x 48 x 32 x 32 floats = 62.9 MB), which the stock formulation holds several times over.  (One matrix path:
    the user encoder has no weight-operand product for ops.BX3 to move.)"""
    from nnr_amd import ops
    case = GoldenCase(FULL)
    model, cfg = build_model(case, 'train')
    b = case.batch('cuda')
    with torch.no_grad():
        cand = model.news_encoder(b[15], b[16], b[17], b[18], b[19], b[20], b[13], b[14], None)
        hist = model.news_encoder(b[3], b[4], b[5], b[6], b[7], b[8], b[1], b[2], None)
    cand, hist = tuple(t.detach().requires_grad_() for t in cand), tuple(t.detach().requires_grad_() for t in hist)
    ue = model.user_encoder
    ue.encode_user(hist, None, None, None, None, cand).sum().backward()           # (first call: workspaces, derived weights)
    ops.join_extra_streams()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ue.encode_user(hist, None, None, None, None, cand).sum().backward()
    ops.join_extra_streams()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print('peak extra allocation %.1f MB (one dense first-layer output: %.1f MB)' % (extra / 1e6, DENSE_A_BYTES / 1e6))
    assert extra < DENSE_A_BYTES


@pytest.mark.parametrize('side', [False, True], ids=['sequential', 'side_stream'])
def test_backward_twice_gives_identical_bits(side):
    """The whole model at the default shapes: two passes from zeroed gradients give the same logits and the same bits in EVERY gradient.
    side_stream: the branch a batch-64 step takes (forced by the threshold) -- the candidate call and its backward on a side stream next to
    the history call's, so the plain read-modify-write writers of both calls (LayerNorm affine gradients, weight unpack) must be ordered."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(FULL)
    old = ops.LEAF_MIN_ROWS
    if side:
        ops.LEAF_MIN_ROWS = 1
    try:
        model, cfg = build_model(case, 'train')
        runs = []
        for _ in range(3 if side else 2):
            for p in model.parameters():
                p.grad = None
            logits = model(*case.batch('cuda'))
            negative_log_softmax(logits).backward()
            ops.join_extra_streams()
            torch.cuda.synchronize()
            runs.append((logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    finally:
        ops.LEAF_MIN_ROWS = old
    for r in runs[1:]:
        assert torch.equal(runs[0][0], r[0])
        for k in runs[0][1]:
            assert float(runs[0][1][k].abs().max()) > 0 and torch.equal(runs[0][1][k], r[1][k]), k
    if side:                      # and the branch computes what the sequential one does
        case2, st, out = restated(FULL)
        for k, g in runs[0][1].items():
            if k.startswith('user_encoder.news_encoder.'):
                continue
            exp, act = case.expect_grad(k, g)
            s = float(st[ZERO_ON_PAPER.get(k, k)].grad.abs().max())
            assert float(np.abs(act.astype(np.float64) - exp).max()) <= BAR * s, k


def test_side_stream_branch_equals_the_sequential_one():
    """Model.forward issues the candidate call on a side stream when the step counts as GPU-bound (forced by the threshold): the join
    carries the (d0, dL) pair."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(TINY[0])
    old = ops.LEAF_MIN_ROWS
    out = []
    try:
        for rows in (1, old):
            ops.LEAF_MIN_ROWS = rows
            model, cfg = build_model(case, 'train')
            logits = model(*case.batch('cuda'))
            negative_log_softmax(logits).backward()
            ops.join_extra_streams()
            torch.cuda.synchronize()
            out.append((logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    finally:
        ops.LEAF_MIN_ROWS = old
    _close('logits', out[0][0], case.expect('f64/logits'), BAR)
    for k in out[0][1]:
        s = float(out[1][1][k].abs().max())
        assert float((out[0][1][k] - out[1][1][k]).abs().max()) <= 1e-5 * max(s, 1e-6), k


@pytest.mark.parametrize('bx3', [True, False], ids=['bx3', 'f32_mfma'])
def test_compute_scores_and_metrics_match_reference(bx3):
    """evaluate.py's per-batch form (the pair's representation is not cacheable) gives the reference's scores, ranks and metrics."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture('tiny_HDC_FIM')
    model = model.cuda().train()
    assert not E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    from nnr_amd import ops
    before = ops.BX3[0]
    ops.BX3[0] = bx3
    try:
        scores = E.compute_scores(model, dc, batch_size=int(z['batch_size']))
    finally:
        ops.BX3[0] = before
    assert model.training and E.LAST_STATS['mode'] == 'per-sample'
    got = scores.cpu().numpy()
    err, smax = float(np.abs(got - z['scores']).max()), float(np.abs(z['scores']).max())
    print('eval_tiny_HDC_FIM scores max-abs-err %.3e (max |score| %.3e)' % (err, smax))
    assert err <= BAR * smax
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
