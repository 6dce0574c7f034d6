"""The small kernels between the big ones on the step's critical chain, entry point by entry point, against fp64 restatements written
here (run with -m gpu on the MI355X box):

  csrc/fuse.hip   nnr_click_loss, nnr_fusion_rows_fwd, nnr_fusion_rows_bwd_det, nnr_fusion_rows_bwd
  csrc/misc.hip   nnr_sue_x0_fwd, nnr_sue_x0_bwd, nnr_sue_slice_fwd, nnr_sue_slice_bwd, nnr_logits_loss_fwd, nnr_rowdot, nnr_add2d,
                  nnr_add_atomic, nnr_relu_bwd
  csrc/dp.hip     nnr_rows_touch, nnr_rows_compact, nnr_rows_pack, nnr_rows_unpack

Shapes are the smallest that reach each code path (capped grids, second lane trips, clamped lanes, the atomic fusion-row form that no
configuration reaches).  Every output starts as NaN (or as a pattern where the kernel accumulates), every output buffer carries guard
elements that must keep their bits, and dropout masks come from nnr_dropout on ones (pinned by test_site_masks_equal_the_kernels_own_masks).
Bars: `close` at 2e-5 of the scale (logits, gradients, table gradients), 2e-6 for the loss, bit equality for pure moves."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def close(actual, expect, tol=2e-5, what=''):
    a = actual.detach().double().cpu()
    e = expect.detach().double().cpu()
    scale = max(1.0, float(e.abs().max()))
    err = float((a - e).abs().max())
    assert err <= tol * scale, '%s: max err %.3e (scale %.3e)' % (what, err, scale)      # (a NaN in `actual` fails too: NaN <= x is False)


def same_bits(a, b):
    """Bit equality that also holds between NaNs (torch.equal calls NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


GUARD = 64


def guarded(*shape, fill=float('nan')):
    """A contiguous fp32 tensor of `shape` cut out of a larger buffer with GUARD elements on either side, and a check that the guard
    elements still hold `fill`'s bits."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device=dev(), dtype=torch.float32)
    ref = buf[:GUARD].clone()
    t = buf[GUARD:GUARD + n].view(*shape)

    def guards_untouched():
        return same_bits(buf[:GUARD], ref) and same_bits(buf[GUARD + n:], ref)
    return t, guards_untouched


def all_nan(t):
    return bool(torch.isnan(t).all())


def pattern(*shape):
    """A non-zero fill for accumulators: += must keep it, = must not."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 7) * 0.25 + 0.5).view(*shape)


def keep_mask(numel, p, seed):
    """The counter-based dropout mask over a flat index: 0 or 1 / (1 - p) in fp32, from nnr_dropout itself."""
    from nnr_amd import ops
    return ops.dropout(torch.ones(numel, device=dev()), p, seed).cpu()


# ------------------------------------------------------------------------------------------------ 1. click predictor + loss
CLICK_SHAPES = [(1, 1, 1), (3, 5, 400), (300, 2, 70), (7, 64, 33)]


def click_inputs(B, N, D, seed=0):
    return rnd(B, N, D, seed=seed + 1, scale=0.1), rnd(B, N, D, seed=seed + 2, scale=0.3)


def click_ref(user, cand):
    """fp64: logits, loss, dlogits, duser, dcand (model.py:126-127, trainer.py:64-66)."""
    ur, cr = user.double().requires_grad_(True), cand.double().requires_grad_(True)
    lg = (ur * cr).sum(2)
    lg.retain_grad()
    loss = -(torch.log_softmax(lg, 1)[:, 0]).mean()
    loss.backward()
    return lg.detach(), loss.detach(), lg.grad, ur.grad, cr.grad


def run_click(user, cand, dlogits=True, grads=True, tail_rows=5):
    """nnr_click_loss into NaN outputs; dcand is the leading B * N rows of a [B * N + tail_rows, D] buffer (step.py's drep[:n0])."""
    from nnr_amd import ops
    B, N, D = user.shape
    d = dev()
    logits, g0 = guarded(B, N)
    loss, g1 = guarded(1)
    dl, g2 = guarded(B, N) if dlogits else (None, lambda: True)
    du, g3 = guarded(B, N, D) if grads else (None, lambda: True)
    drep, g4 = guarded(B * N + tail_rows, D) if grads else (None, lambda: True)
    dc = drep[:B * N] if grads else None
    terms = torch.full((B,), float('nan'), device=d)
    ops.click_loss(user.to(d), cand.to(d), B, N, D, logits, loss, dl, du, dc, terms)
    torch.cuda.synchronize()
    assert g0() and g1() and g2() and g3() and g4(), 'click_loss wrote outside its outputs'
    if grads:
        assert all_nan(drep[B * N:]), 'click_loss wrote past the candidate rows of the gradient buffer'
        dc = dc.view(B, N, D)
    return logits, loss, dl, du, dc


@pytest.mark.parametrize('B,N,D', CLICK_SHAPES)
def test_click_loss_matches_fp64(B, N, D):
    user, cand = click_inputs(B, N, D)
    lg, loss_ref, dl_ref, du_ref, dc_ref = click_ref(user, cand)
    logits, loss, dl, du, dc = run_click(user, cand)
    close(logits, lg, what='click logits')
    close(loss.view(()), loss_ref, tol=2e-6, what='click loss')
    close(dl, dl_ref, what='click dlogits')
    close(du, du_ref, what='click duser')
    close(dc, dc_ref, what='click dcand')
    if (B, N, D) == (1, 1, 1):
        assert float(loss) == 0.0 and float(dl) == 0.0
    # dlogits = None: everything else as before
    l2, loss2, _, du2, dc2 = run_click(user, cand, dlogits=False)
    assert torch.equal(l2, logits) and torch.equal(loss2, loss) and torch.equal(du2, du) and torch.equal(dc2, dc)
    # forward only
    l3, loss3, dl3, _, _ = run_click(user, cand, grads=False)
    assert torch.equal(l3, logits) and torch.equal(loss3, loss) and torch.equal(dl3, dl)


@pytest.mark.parametrize('B,N,D', CLICK_SHAPES)
def test_logits_loss_fwd_matches_fp64_and_the_separate_launches(B, N, D):
    """nnr_logits_loss_fwd = nnr_logits_fwd + nnr_nls_loss, same bits."""
    from nnr_amd import ops
    d = dev()
    user, cand = click_inputs(B, N, D, seed=10)
    lg, loss_ref, dl_ref, _, _ = click_ref(user, cand)
    ud, cd = user.to(d), cand.to(d)
    logits, g0 = guarded(B, N)
    loss, g1 = guarded(1)
    dl, g2 = guarded(B, N)
    ops.logits_loss_fwd(ud, cd, B, N, D, logits, loss, dl)
    close(logits, lg, what='logits_loss_fwd logits')
    close(loss.view(()), loss_ref, tol=2e-6, what='logits_loss_fwd loss')
    close(dl, dl_ref, what='logits_loss_fwd dlogits')
    assert g0() and g1() and g2()
    l2, loss2, dl2 = guarded(B, N)[0], guarded(1)[0], guarded(B, N)[0]
    ops.logits_fwd(ud, cd, B, N, D, l2)
    ops.nls_loss(l2, B, N, loss2, dl2)
    assert torch.equal(l2, logits) and torch.equal(loss2, loss) and torch.equal(dl2, dl)
    loss3, g3 = guarded(1)
    ops.logits_loss_fwd(ud, cd, B, N, D, logits, loss3, None)                     # dlogits = None
    assert torch.equal(loss3, loss) and g3()


@pytest.mark.parametrize('B,N,D', CLICK_SHAPES)
def test_click_loss_is_bit_identical_to_the_three_launches_it_replaces(B, N, D):
    """The promise in the header of csrc/fuse.hip: nnr_click_loss = nnr_logits_fwd + nnr_nls_loss + nnr_logits_bwd, bit for bit."""
    from nnr_amd import ops
    d = dev()
    user, cand = click_inputs(B, N, D, seed=20)
    logits, loss, dl, du, dc = run_click(user, cand)
    ud, cd = user.to(d), cand.to(d)
    l2, loss2, dl2 = guarded(B, N)[0], guarded(1)[0], guarded(B, N)[0]
    du2, dc2 = guarded(B, N, D)[0], guarded(B, N, D)[0]
    ops.logits_fwd(ud, cd, B, N, D, l2)
    ops.nls_loss(l2, B, N, loss2, dl2)
    ops.logits_bwd(dl2, ud, cd, B, N, D, du2, dc2)
    for name, a, b in (('logits', logits, l2), ('loss', loss, loss2), ('dlogits', dl, dl2), ('duser', du, du2), ('dcand', dc, dc2)):
        assert torch.equal(a, b), '%s differs from the unfused launches: max |diff| %.3e' % (name, float((a - b).abs().max()))


def test_click_loss_is_stable_at_large_logits():
    """Logits reach +-150: exp(150) overflows fp32, so a softmax without the max subtraction gives inf / NaN here."""
    B, N, D = 3, 5, 400
    user, cand = click_inputs(B, N, D, seed=30)
    lg = (user.double() * cand.double()).sum(2)
    user = (user.double() * (150.0 / float(lg.abs().max()))).float()
    lg, loss_ref, dl_ref, du_ref, dc_ref = click_ref(user, cand)
    assert 149.0 < float(lg.abs().max()) < 151.0 and float(lg.min()) < -100.0 and float(lg.max()) > 100.0
    logits, loss, dl, du, dc = run_click(user, cand)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
    close(logits, lg, what='large logits')
    close(loss.view(()), loss_ref, tol=2e-6, what='loss at large logits')
    close(dl, dl_ref, what='dlogits at large logits')
    close(du, du_ref, what='duser at large logits')
    close(dc, dc_ref, what='dcand at large logits')


def test_click_loss_arrival_counter_is_reset_between_launches():
    """B = 300, 1, 7 back to back on one stream without a synchronisation between them: the process-wide arrival counter must be back
    at zero when the next grid (of another size) starts, or that grid never sees its last workgroup / sees it too early."""
    from nnr_amd import ops
    d = dev()
    cases = []
    for i, (B, N, D) in enumerate(((300, 2, 70), (1, 3, 9), (7, 5, 33))):
        user, cand = click_inputs(B, N, D, seed=40 + i)
        cases.append((user, cand, user.to(d), cand.to(d), torch.full((B, N), float('nan'), device=d), torch.full((1,), float('nan'), device=d),
                      torch.full((B,), float('nan'), device=d)))
    torch.cuda.synchronize()
    for user, cand, ud, cd, logits, loss, terms in cases:
        B, N, D = user.shape
        ops.click_loss(ud, cd, B, N, D, logits, loss, None, None, None, terms)
    torch.cuda.synchronize()
    for user, cand, ud, cd, logits, loss, terms in cases:
        lg, loss_ref, _, _, _ = click_ref(user, cand)
        close(logits, lg, what='logits, B=%d' % user.shape[0])
        close(loss.view(()), loss_ref, tol=2e-6, what='loss of the launch with B=%d' % user.shape[0])


def test_click_loss_refuses_what_it_cannot_run():
    from nnr_amd import _lib as L, ops
    d = dev()
    for (B, N, D, half) in ((2, 65, 8, False), (2, 5, 8, True)):             # N > CLICK_MAXN; duser without dcand
        user, cand = click_inputs(B, N, D, seed=50)
        logits, loss, dl, du, dc = (torch.full(s, float('nan'), device=d) for s in ((B, N), (1,), (B, N), (B, N, D), (B, N, D)))
        with pytest.raises(L.NnrHipError):
            ops.click_loss(user.to(d), cand.to(d), B, N, D, logits, loss, dl, du, None if half else dc, torch.full((B,), float('nan'), device=d))
        torch.cuda.synchronize()
        assert all(all_nan(t) for t in (logits, loss, dl, du, dc))


# ------------------------------------------------------------------------------------------------ 2. feature-fusion rows
GEOMETRIES = [(18, 50, 270, 50), (5, 128, 7, 64), (4, 65, 3, 1), (6, 3, 9, 129)]       # (ncat, cd, nsub, sd)
WIDE = (6, 3, 9, 129)
FUSION_CASES = [(g, c) for g in GEOMETRIES for c in ((50, 0), (37, 203), (1500, 1000))] + [(WIDE, (3000, 14000))]


def history_ids(n, rows, gen):
    """History-shaped ids over a table of `rows` rows: every 50-row block ends in a run of id 0 (padded history slots), row
    rows - 2 of the table never occurs and row rows - 1 occurs exactly once, as the very last id."""
    ids = torch.randint(0, rows - 2, (n,), generator=gen).int()
    for u0 in range(0, n, 50):
        ids[u0 + int(torch.randint(5, 50, (1,), generator=gen)):u0 + 50] = 0
    ids[n - 1] = rows - 1
    return ids


_FUSION = {}


def fusion_case(geom, call, p):
    """Inputs and the fp64 reference of one (geometry, call shape, p), built once and shared by the forward and backward tests."""
    key = (geom, call, p)
    if key not in _FUSION:
        ncat, cd, nsub, sd = geom
        n0, n1 = call
        n = n0 + n1
        gen = torch.Generator().manual_seed(1000 * n + cd)
        cat, sub = history_ids(n, ncat, gen), history_ids(n, nsub, gen)
        ctab, stab = rnd(ncat, cd, seed=61), rnd(nsub, sd, seed=62)
        seed_c, seed_s = 4242, 777
        # mask index row * dim + c over the UNION of the two calls: the second call's row r is row n0 + r
        mc = keep_mask(n * cd, p, seed_c).view(n, cd).double()
        ms = keep_mask(n * sd, p, seed_s).view(n, sd).double()
        fwd = torch.cat([ctab.double()[cat.long()] * mc, stab.double()[sub.long()] * ms], 1)
        dout = rnd(n, 3 + cd + sd + 2, seed=63)
        dview = dout[:, 3:3 + cd + sd].double()
        dct = pattern(ncat, cd).double().index_add_(0, cat.long(), dview[:, :cd] * mc)
        dst = pattern(nsub, sd).double().index_add_(0, sub.long(), dview[:, cd:] * ms)
        _FUSION[key] = dict(cat=cat, sub=sub, ctab=ctab, stab=stab, seeds=(seed_c, seed_s), fwd=fwd, dout=dout, dct=dct, dst=dst)
    return _FUSION[key]


def split_ids(ids, n0, n1):
    d = dev()
    return ids[:n0].contiguous().to(d), (ids[n0:].contiguous().to(d) if n1 else None)


@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('geom,call', FUSION_CASES)
def test_fusion_rows_forward(geom, call, p):
    """nnr_fusion_rows_fwd = table[id] * mask into a column view of a wider buffer."""
    from nnr_amd import ops
    d = dev()
    (ncat, cd, nsub, sd), (n0, n1) = geom, call
    n, w = n0 + n1, cd + sd
    k = fusion_case(geom, call, p)
    cat0, cat1 = split_ids(k['cat'], n0, n1)
    sub0, sub1 = split_ids(k['sub'], n0, n1)
    ld = 3 + w + 2
    wide, guards = guarded(n, ld)
    ops.fusion_rows_fwd(k['ctab'].to(d), k['stab'].to(d), cat0, sub0, cat1, sub1, wide[:, 3:], ld, p, *k['seeds'])
    torch.cuda.synchronize()
    assert guards() and all_nan(wide[:, :3]) and all_nan(wide[:, 3 + w:]), 'columns outside the view were written'
    out = wide[:, 3:3 + w]
    if p == 0.0:
        assert torch.equal(out.cpu(), torch.cat([k['ctab'][k['cat'].long()], k['stab'][k['sub'].long()]], 1))        # a pure move
    else:
        close(out, k['fwd'], what='fusion rows fwd')
    if n1 == 0:                                      # one call: the two launches it replaces, same seeds, same bits
        two = torch.full((n, ld), float('nan'), device=d)
        ops.small_embed_fwd(k['ctab'].to(d), cat0, two[:, 3:], ld, p, k['seeds'][0])
        ops.small_embed_fwd(k['stab'].to(d), sub0, two[:, 3 + cd:], ld, p, k['seeds'][1])
        assert torch.equal(two[:, 3:3 + w], out)


@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('geom,call', FUSION_CASES)
def test_fusion_rows_backward(geom, call, p):
    """ops.fusion_rows_bwd: nnr_fusion_rows_bwd_det (tables up to 128 wide: reproducible) or nnr_fusion_rows_bwd (wider: run-merging
    f32 atomics) adds dout_view * mask into the rows of two table gradients that already hold something."""
    from nnr_amd import ops
    d = dev()
    (ncat, cd, nsub, sd), (n0, n1) = geom, call
    k = fusion_case(geom, call, p)
    cat0, cat1 = split_ids(k['cat'], n0, n1)
    sub0, sub1 = split_ids(k['sub'], n0, n1)
    dout = k['dout'].to(d)
    ld = dout.shape[1]
    runs = []
    for _ in range(2):
        dct, gc = guarded(ncat, cd)
        dst, gs = guarded(nsub, sd)
        dct.copy_(pattern(ncat, cd))
        dst.copy_(pattern(nsub, sd))
        ops.fusion_rows_bwd(cat0, sub0, cat1, sub1, cd, sd, dout[:, 3:], ld, dct, dst, p, *k['seeds'])
        torch.cuda.synchronize()
        assert gc() and gs(), 'wrote outside the table gradients'
        close(dct, k['dct'], what='category table gradient')
        close(dst, k['dst'], what='subCategory table gradient')
        assert torch.equal(dct[ncat - 2].cpu(), pattern(ncat, cd)[ncat - 2]) and torch.equal(dst[nsub - 2].cpu(), pattern(nsub, sd)[nsub - 2]), \
            'the row of an id that does not occur changed'
        runs.append((dct.clone(), dst.clone()))
    if cd <= 128 and sd <= 128:                      # the reproducible form; the atomic form is held to the fp64 bar only
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_fusion_rows_backward_atomic_form_on_the_narrow_geometries():
    """nnr_fusion_rows_bwd called directly: ops.fusion_rows_bwd only picks it for tables wider than 128, the kernel itself has no such limit."""
    from nnr_amd import _lib as L, ops
    d = dev()
    for geom in GEOMETRIES[:3]:
        (ncat, cd, nsub, sd), (n0, n1), p = geom, (1500, 1000), 0.3
        k = fusion_case(geom, (n0, n1), p)
        cat0, cat1 = split_ids(k['cat'], n0, n1)
        sub0, sub1 = split_ids(k['sub'], n0, n1)
        dout = k['dout'].to(d)
        dct, gc = guarded(ncat, cd)
        dst, gs = guarded(nsub, sd)
        dct.copy_(pattern(ncat, cd))
        dst.copy_(pattern(nsub, sd))
        L.check(L.lib().nnr_fusion_rows_bwd(ops._p(cat0), ops._p(sub0), n0, ops._p(cat1), ops._p(sub1), n1, cd, sd, ops._p(dout[:, 3:]), dout.shape[1],
                                            ops._p(dct), ops._p(dst), C.c_float(p), C.c_uint32(k['seeds'][0]), C.c_uint32(k['seeds'][1]), ops._s()),
                'nnr_fusion_rows_bwd')
        torch.cuda.synchronize()
        assert gc() and gs()
        close(dct, k['dct'], what='category table gradient, atomic form %s' % (geom,))
        close(dst, k['dst'], what='subCategory table gradient, atomic form %s' % (geom,))


# ------------------------------------------------------------------------------------------------ 3. SUE graph input and slices
SUE_SHAPES = [(3, 5, 2, 20), (2, 50, 19, 400), (40, 50, 19, 300)]       # (B, Hn, Kc, D); the last: B * G * D > 2048 * 256


@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('B,Hn,Kc,D', SUE_SHAPES)
def test_sue_x0_forward(B, Hn, Kc, D, p):
    """nnr_sue_x0_fwd: X0[b, :Hn] = hist[b]; X0[b, Hn + k] = proxy[k] * mask[b, k] (mask index ((b * Kc + k) * D + c))."""
    from nnr_amd import ops
    d = dev()
    G, seed = Hn + Kc, 991
    hist, proxy = rnd(B, Hn, D, seed=70), rnd(Kc, D, seed=71)
    mask = keep_mask(B * Kc * D, p, seed).view(B, Kc, D)
    if p > 0:
        assert not torch.equal(mask[0], mask[1]), 'the proxy mask must differ between samples'
    x0, guards = guarded(B, G, D)
    cmask = torch.zeros(B, Kc + 1, dtype=torch.uint8, device=d)
    ops.sue_x0_fwd(hist.to(d), proxy.to(d), x0, B, Hn, Kc, D, p, seed, cmask_fix=cmask)
    torch.cuda.synchronize()
    assert guards()
    assert torch.equal(x0[:, :Hn].cpu(), hist)
    close(x0[:, Hn:], proxy.double().unsqueeze(0) * mask.double(), what='proxy rows')
    if p == 0:
        assert torch.equal(x0[:, Hn:].cpu(), proxy.unsqueeze(0).expand(B, Kc, D))
    else:
        assert torch.equal(x0[:, Hn:].cpu() == 0, mask == 0)
    want = torch.zeros(B, Kc + 1, dtype=torch.uint8)
    want[:, Kc] = 1
    assert torch.equal(cmask.cpu(), want)
    x1, guards1 = guarded(B, G, D)
    ops.sue_x0_fwd(hist.to(d), proxy.to(d), x1, B, Hn, Kc, D, p, seed, cmask_fix=None)           # no mask to fix: same X0
    torch.cuda.synchronize()
    assert torch.equal(x1, x0) and guards1()


@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('B,Hn,Kc,D', SUE_SHAPES)
def test_sue_x0_backward(B, Hn, Kc, D, p, with_add):
    """nnr_sue_x0_bwd: dhist = (dX0 + dX0_add)[:, :Hn]; dproxy[k] += sum_b mask[b, k] * (dX0 + dX0_add)[b, Hn + k], in sample order."""
    from nnr_amd import ops
    d = dev()
    G, seed = Hn + Kc, 992
    dx0 = rnd(B, G, D, seed=72).to(d)
    add = rnd(B, G, D, seed=73).to(d) if with_add else None
    up = dx0 + add if with_add else dx0                      # one fp32 add per element: correctly rounded, the same bits everywhere
    mask = keep_mask(B * Kc * D, p, seed).view(B, Kc, D).double()
    want = pattern(Kc, D).double() + (up[:, Hn:].cpu().double() * mask).sum(0)
    runs = []
    for _ in range(2):
        dhist, gh = guarded(B, Hn, D)
        dproxy, gp = guarded(Kc, D)
        dproxy.copy_(pattern(Kc, D))
        ops.sue_x0_bwd(dx0, dhist, dproxy, B, Hn, Kc, D, p, seed, dx0_add=add)
        torch.cuda.synchronize()
        assert gh() and gp()
        assert torch.equal(dhist, up[:, :Hn])
        close(dproxy, want, what='dproxy')
        runs.append(dproxy.clone())
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize('B,Hn,Kc,D', SUE_SHAPES)
def test_sue_slices(B, Hn, Kc, D):
    """nnr_sue_slice_fwd: gfeat = (gcn + X0)[:, :Hn]; nnr_sue_slice_bwd: dpad[:, :Hn] = dgfeat, dpad[:, Hn:] = 0."""
    from nnr_amd import ops
    d = dev()
    G = Hn + Kc
    gcn, x0 = rnd(B, G, D, seed=74).to(d), rnd(B, G, D, seed=75).to(d)
    gfeat, gg = guarded(B, Hn, D)
    ops.sue_slice_fwd(gcn, x0, gfeat, B, Hn, G, D)
    torch.cuda.synchronize()
    assert gg() and torch.equal(gfeat, (gcn + x0)[:, :Hn])
    dgfeat = rnd(B * Hn + 1, D, seed=76).to(d)[:B * Hn].view(B, Hn, D)       # (one spare row behind it: an off-by-one row read stays inside the buffer)
    dpad, gd = guarded(B, G, D)
    ops.sue_slice_bwd(dgfeat, dpad, B, Hn, G, D)
    torch.cuda.synchronize()
    assert gd() and torch.equal(dpad[:, :Hn], dgfeat)
    assert torch.equal(dpad[:, Hn:], torch.zeros(B, Kc, D, device=d)), 'proxy rows of the padded gradient must be exactly 0'


# ------------------------------------------------------------------------------------------------ 4. rowdot, add2d, add_atomic_, relu_bwd
@pytest.mark.parametrize('rows,N,ld', [(5, 4, 4), (37, 200, 208), (130, 260, 260), (33000, 8, 8)])
def test_rowdot_standalone(rows, N, ld):
    """nnr_rowdot: out[row] = <x[row, :N], w>, float4 lanes (a second trip past 64 float4s), a device row count, a row loop under the
    8192-block cap."""
    from nnr_amd import ops
    d = dev()
    xb, w = rnd(rows, ld, seed=80), rnd(N, seed=81)
    x = xb.to(d)[:, :N]
    want = xb[:, :N].double() @ w.double()
    for live in (None, rows - max(1, rows // 3), rows + 5):
        out, guards = guarded(rows)
        dyn = None if live is None else torch.tensor([live], dtype=torch.int32, device=d)
        ops.rowdot(x, w.to(d), out, dyn=dyn)
        torch.cuda.synchronize()
        R = rows if live is None else min(rows, live)
        assert guards()
        close(out[:R], want[:R], what='rowdot, live rows %s' % live)
        assert all_nan(out[R:]), 'rows at and beyond the device count were written'


def test_rowdot_refuses_unaligned_inputs():
    from nnr_amd import _lib as L, ops
    d = dev()
    out = torch.full((5,), float('nan'), device=d)
    wb = torch.ones(16, device=d)
    with pytest.raises(L.NnrHipError, match='code -3'):              # NNR_ERR_UNSUPPORTED
        ops.rowdot(torch.ones(5, 8, device=d)[:, :6], wb[:6], out)
    with pytest.raises(L.NnrHipError, match='code -3'):
        ops.rowdot(torch.ones(5, 8, device=d), wb[1:9], out)
    torch.cuda.synchronize()
    assert all_nan(out)


@pytest.mark.parametrize('alpha', [1.0, -0.5])
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('rows,cols', [(7, 3), (1100, 500)])
def test_add2d_between_column_views(rows, cols, accumulate, alpha):
    """nnr_add2d: y[:, :cols] (+)= alpha * x[:, :cols] between column views of buffers with different leading dimensions, as feature
    fusion copies the representation in and its gradient out."""
    from nnr_amd import ops
    ldx, ldy = cols + 5, cols + 9
    xb = rnd(rows, ldx, seed=82)
    yb, guards = guarded(rows, ldy)
    if accumulate:
        yb.copy_(pattern(rows, ldy))
    before = yb.clone()
    x = xb.to(dev())
    ops.add2d(yb[:, 4:], ldy, x[:, 2:], ldx, rows, cols, alpha=alpha, accumulate=accumulate)
    torch.cuda.synchronize()
    assert guards() and same_bits(yb[:, :4], before[:, :4]) and same_bits(yb[:, 4 + cols:], before[:, 4 + cols:]), 'guard columns changed'
    got, src = yb[:, 4:4 + cols], xb[:, 2:2 + cols]
    if alpha == 1.0 and not accumulate:
        assert torch.equal(got.cpu(), src)                                      # a pure move
    else:
        base = pattern(rows, ldy)[:, 4:4 + cols].double() if accumulate else 0.0
        close(got, base + alpha * src.double(), what='add2d')


def test_add_atomic_from_two_streams():
    """nnr_add_atomic: two launches on two streams of the package into one accumulator."""
    from nnr_amd import ops
    d = dev()
    n = 1_048_579
    a, b = rnd(n, seed=83), rnd(n, seed=84)
    acc, guards = guarded(n)
    acc.copy_(pattern(n))
    ad, bd = a.to(d), b.to(d)
    had = list(ops.EXTRA_STREAMS)
    cur = torch.cuda.current_stream(d)
    s1, s2 = ops.new_stream(d), ops.new_stream(d)
    try:
        for st, x, alpha in ((s1, ad, 1.0), (s2, bd, -0.5)):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                ops.add_atomic_(acc, x, alpha)
        cur.wait_stream(s1)
        cur.wait_stream(s2)
        torch.cuda.synchronize()
    finally:
        ops.EXTRA_STREAMS[:] = had
    assert guards()
    close(acc, pattern(n).double() + a.double() - 0.5 * b.double(), what='add_atomic_ from two streams')


def test_relu_bwd_is_exact():
    """nnr_relu_bwd: dx = dy where y > 0, exactly 0 elsewhere (y = 0, -0, negative)."""
    from nnr_amd import ops
    d = dev()
    n = 524_291
    y, dy = rnd(n, seed=85), rnd(n, seed=86)
    y[::3] = 0.0
    y[1::7] = -0.0
    dx, guards = guarded(n)
    ops.relu_bwd(dy.to(d), y.to(d), dx)
    torch.cuda.synchronize()
    assert guards()
    assert same_bits(dx.cpu(), torch.where(y > 0, dy, torch.zeros(n)))


# ------------------------------------------------------------------------------------------------ 5. touched-row exchange
ROWS_SIZES = [(5, 1), (1024, 65), (1025, 300), (60001, 300)]
TOUCHED = ['none', 'all', 'first', 'last', 'random']


def touched_set(V, kind):
    t = np.zeros(V, dtype=bool)
    if kind == 'all':
        t[:] = True
    elif kind == 'first':
        t[0] = True
    elif kind == 'last':
        t[V - 1] = True
    elif kind == 'random':
        t[np.random.default_rng(V).random(V) < 0.03] = True
        if not t.any():
            t[V // 2] = True
    return t


def token_stream(V, touched, rng):
    """Live tokens that hit exactly the touched rows (each at least once, some often) between ids the kernel must ignore."""
    rows = np.flatnonzero(touched)
    live = np.concatenate([rows, rng.choice(rows, size=2 * len(rows) + 3) if len(rows) else rows[:0], np.array([-1, V, V + 7] * 3)])
    return rng.permutation(live).astype(np.int32)


def rows_api():
    from nnr_amd import _lib as L, ops
    return L, ops


def run_touch_compact(V, touched, mode):
    """nnr_rows_touch + nnr_rows_compact as nnr_amd/dp.py calls them.  mode: 'none' (no device count), 'below' (device count < cap; the
    tokens past it name untouched rows), 'above' (device count > cap: clamps; the ids behind the view name untouched rows too)."""
    L, ops = rows_api()
    d = dev()
    rng = np.random.default_rng(V + len(mode))
    live = token_stream(V, touched, rng)
    other = np.flatnonzero(~touched)
    dead = rng.choice(other, size=200).astype(np.int32) if len(other) else np.full(200, -1, dtype=np.int32)
    buf = torch.from_numpy(np.concatenate([live, dead])).to(d)
    if mode == 'below':
        tok, total = buf, torch.tensor([len(live)], dtype=torch.int32, device=d)
    else:
        tok = buf[:len(live)]
        total = None if mode == 'none' else torch.tensor([len(live) + 50], dtype=torch.int32, device=d)
    flags, gf = guarded(V, fill=0.0)
    pos = torch.full((V + 2 * GUARD,), -7, dtype=torch.int32, device=d)
    count = torch.full((3,), -7, dtype=torch.int32, device=d)
    L.check(L.lib().nnr_rows_touch(ops._p(tok), C.c_long(tok.numel()), ops._p(total), V, ops._p(flags), ops._s()), 'nnr_rows_touch')
    L.check(L.lib().nnr_rows_compact(ops._p(flags), V, ops._p(pos[GUARD:]), ops._p(count[1:]), ops._s()), 'nnr_rows_compact')
    torch.cuda.synchronize()
    assert gf() and bool((pos[:GUARD] == -7).all()) and bool((pos[GUARD + V:] == -7).all()) and count[0].item() == -7 and count[2].item() == -7
    return flags, pos[GUARD:GUARD + V], count[1:2]


@pytest.mark.parametrize('mode', ['none', 'below', 'above'])
@pytest.mark.parametrize('kind', TOUCHED)
@pytest.mark.parametrize('V', [v for v, _ in ROWS_SIZES])
def test_rows_touch_and_compact(V, kind, mode):
    touched = touched_set(V, kind)
    flags, pos, count = run_touch_compact(V, touched, mode)
    assert np.array_equal(flags.cpu().numpy(), touched.astype(np.float32))
    want = np.where(touched, np.cumsum(touched) - touched, -1).astype(np.int32)
    assert np.array_equal(pos.cpu().numpy(), want)
    assert int(count.item()) == int(touched.sum())


@pytest.mark.parametrize('kind', TOUCHED)
@pytest.mark.parametrize('V,E', ROWS_SIZES)
def test_rows_pack_and_unpack(V, E, kind):
    """nnr_rows_pack: packed[pos[w]] = dense[w]; nnr_rows_unpack: dense[w] = packed[pos[w]]; touched rows only, pure moves."""
    L, ops = rows_api()
    d = dev()
    touched = touched_set(V, kind)
    _, pos, count = run_touch_compact(V, touched, 'none')
    U = int(count.item())
    assert U == int(touched.sum())
    rows = torch.from_numpy(np.flatnonzero(touched)).to(d)
    dense = torch.randn(V, E, device=d, generator=torch.Generator(device=d).manual_seed(V + E))
    packed, gp = guarded(U + 3, E)
    L.check(L.lib().nnr_rows_pack(ops._p(dense), ops._p(pos), V, E, ops._p(packed), ops._s()), 'nnr_rows_pack')
    torch.cuda.synchronize()
    assert gp() and torch.equal(packed[:U], dense.index_select(0, rows)) and all_nan(packed[U:])
    back, gb = guarded(V, E)
    L.check(L.lib().nnr_rows_unpack(ops._p(packed), ops._p(pos), V, E, ops._p(back), ops._s()), 'nnr_rows_unpack')
    torch.cuda.synchronize()
    assert gb() and torch.equal(back.index_select(0, rows), dense.index_select(0, rows))
    untouched = torch.from_numpy(np.flatnonzero(~touched)).to(d)
    assert all_nan(back.index_select(0, untouched)), 'unpack wrote a row that is not touched'
