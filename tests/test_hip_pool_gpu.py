"""The masked-softmax attention pool (csrc/pool.hip: nnr_attn_pool_fwd, nnr_attn_pool_bwd) on every path, shape class and stride,
against the float64 restatement of tests/pool_ref.py (run with -m gpu on the MI355X box).

  dispatch     pool_packed_kernel<NV = 1 | 2, R = 8> and pool_kernel<NV = 1 | 2 | 4 | 5>, packed and dense (pool_ref.path_of)
  bodies       single-wave teams (<= 8 tokens, four sequences per workgroup), four-wave teams (9 .. 32), the stream body (> 32), with
               explicit length tables on both sides of 8 | 9, 32 | 33 and 64 | 65 and every fill of the last single-wave workgroup
  scores       GIVEN, DOT, and the fused th . w2 row-dot
  masks        none; packed with the caller's hole mask over a plan built from ops.mask_cover (functional.PackedAttentionFn); dense with
               mask_div = 1 and 3; fully masked groups
  backward     dx plain / accumulated / with dout2, dscore only, dv without dx, a second pool folded into the one write of dx
  strides      every leading dimension distinct and wider than D

Conventions of test_hip_fused_tail_gpu.py: every output starts as NaN (or as pattern() where the kernel accumulates) and is cut from a
buffer with guard elements; guards, the gap columns of a wide row and the packed rows at or beyond the plan's total must keep their bits;
those rows are NaN in x, th, score, alpha and dscore_b, so a pad row that leaks into a result shows.  tests/test_pool_host.py asserts
that the shared case tables reach every path.

Bars: `close` at 2e-5 of max |expected| of the tensor (no floor of 1: alpha at L = 128 is about 0.008).  No case needed a measured bar:
the largest error over all cases is 6.2e-7 of the scale (a dscore; dx and dv at D = 1280 included).  The accumulating form is
compared after the pattern is subtracted again, so it carries the rounding of `pattern + dx` (half an ulp of a value below 4, 1.2e-7)
on top: 4.6e-6 of the scale on the rows of a fully masked sequence at L = 128, whose dx is only dout / 128.
Bit equality only for guards, gaps, pad rows, run-to-run determinism, compact against strided operands, the fold against the two-pass
form's dv / dscore, and dscore == 0.0 on fully masked groups."""
import functools
import types

import numpy as np
import pytest
import torch

import pool_ref as R

pytestmark = pytest.mark.gpu
NAN = float('nan')


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def close(actual, expect, tol=2e-5, what=''):
    a = actual.detach().double().cpu()
    e = expect.detach().double().cpu()
    assert a.shape == e.shape, '%s: shape %s vs %s' % (what, tuple(a.shape), tuple(e.shape))
    scale = float(e.abs().max())
    err = float((a - e).abs().max())
    print('%s: max err %.3e, scale %.3e, ratio %.3e' % (what, err, scale, err / scale if scale else 0.0))
    assert err <= tol * scale, '%s: max err %.3e (scale %.3e)' % (what, err, scale)      # (a NaN in `actual` fails too: NaN <= x is False)


def same_bits(a, b):
    """Bit equality that also holds between NaNs (torch.equal calls NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


GUARD = 64


def pattern(*shape):
    """A non-zero fill for accumulators: += must keep it, = must not."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 7) * 0.25 + 0.5).view(*shape)


class Out:
    """An output [rows, cols] with leading dimension ld, cut from a buffer with GUARD elements on either side; NaN, or pattern() over
    all of [rows, ld].  check(): the guards, the gap columns and the rows the kernel has no business in still hold their bits."""

    def __init__(self, rows, cols, ld=None, fill=NAN):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        n = rows * self.ld
        self.buf = torch.full((n + 2 * GUARD,), NAN, device=dev(), dtype=torch.float32)
        if fill == 'pattern':
            self.buf[GUARD:GUARD + n] = pattern(n).to(dev())
        elif fill == fill:
            self.buf[GUARD:GUARD + n] = fill
        self.full = self.buf[GUARD:GUARD + n].view(rows, self.ld)        # what the kernel gets (its first element)
        self.t = self.full[:, :cols]
        self.before = self.buf.clone()

    def check(self, live_rows=None, what=''):
        torch.cuda.synchronize()
        may = torch.zeros(self.rows, self.ld, dtype=torch.bool)
        if live_rows is None:
            may[:, :self.cols] = True
        else:
            may[live_rows, :self.cols] = True
        g = torch.zeros(GUARD, dtype=torch.bool)
        keep = ~torch.cat([g, may.flatten(), g]).to(dev())
        assert same_bits(self.buf[keep], self.before[keep]), '%s: wrote outside its rows / columns' % what

    def initial(self):
        return self.before[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]


def widen(t, ld):
    """[rows, cols] -> device [rows, ld] with NaN in the gap columns."""
    rows, cols = t.shape
    out = torch.full((rows, ld), NAN, dtype=torch.float32)
    out[:, :cols] = t
    return out.to(dev())


# ------------------------------------------------------------------------------------------------ problems
def problem(n, L, D, lens, mode, A=0, mask=None, mask_div=1, seed=0, plan_from_cover=False):
    """Host operands of one pool call (dense [n, L, .] tensors, fp32) and, for a packed one, its plan.  lens = None: dense."""
    from nnr_amd import ops
    P = types.SimpleNamespace(n=n, L=L, D=D, mode=mode, A=A, mask=mask, mask_div=mask_div, packed=lens is not None, lens=lens)
    P.x = rnd(n, L, D, seed=seed + 1)
    P.v = rnd(n, D, seed=seed + 2, scale=2.0 / D ** 0.5)
    P.scale = 0.5
    P.score = rnd(n, L, seed=seed + 3)
    P.add_in = rnd(n, D, seed=seed + 4)
    P.dout, P.dout2, P.dout_b = rnd(n, D, seed=seed + 5), rnd(n, D, seed=seed + 6), rnd(n, D, seed=seed + 7)
    P.v_b, P.scale_b = rnd(n, D, seed=seed + 8, scale=2.0 / D ** 0.5), 0.31
    if mode == 'th':
        P.th = torch.tanh(rnd(n, L, A, seed=seed + 9))
        P.w2 = rnd(A, seed=seed + 10, scale=2.0 / A ** 0.5)
    P.masked_seqs = [] if mask is None else [s for s in range(n) if not bool(mask[s // mask_div].any())]
    if P.packed:
        lt = torch.tensor(lens)
        P.live = torch.arange(L)[None, :] < lt[:, None]
        if plan_from_cover:                                  # functional.MhsaPack: the plan of the cover, the pool gets the holes
            cover = ops.mask_cover(mask.to(dev()))
            assert torch.equal(cover.cpu().bool(), P.live)
            P.plan = ops.SeqPlan(cover, None)
        else:
            P.plan = ops.SeqPlan(P.live.clone().to(dev()), None)
        assert P.plan.len.cpu().tolist() == lens
        P.rows = R.packed_rows(P.plan.off, P.plan.rank, L)
        P.cap, P.total = P.plan.cap, int(P.plan.off[L])
        assert P.total == sum(lens) and (n == 1 or P.plan.order.cpu().tolist() != list(range(n)))
        P.live_rows = torch.arange(P.cap) < P.total
    else:
        P.live = torch.ones(n, L, dtype=torch.bool)
        P.plan, P.rows, P.cap, P.total = None, None, n * L, n * L
        P.live_rows = None
    return P


def strides(P, **over):
    S = dict(ldx=P.D, ldv=P.D, ldo=P.D, ldadd=P.D, lddo=P.D, lddo2=P.D, lddx=P.D, lddv=P.D, lddo_b=P.D, ldv_b=P.D, ldth=P.A)
    S.update(over)
    return S


def wide_strides(P):
    """Every leading dimension distinct, a multiple of 4 and greater than the row."""
    keys = ('ldx', 'ldv', 'ldo', 'ldadd', 'lddo', 'lddo2', 'lddx', 'lddv', 'lddo_b', 'ldv_b')
    S = {k: P.D + 4 * (i + 1) for i, k in enumerate(keys)}
    S['ldth'] = P.A + 4 * (len(keys) + 1) if P.A else 0
    assert len(set(S.values())) == len(S)
    return S


def tokens(P, dense, ld=None):
    """Per-token operand [n, L] / [n, L, C] -> device [cap] / [cap, ld]: packed rows (NaN at and beyond the total) or s * L + t."""
    if P.packed:
        return R.pack(dense, P.rows, P.live, P.cap, ld=ld).to(dev())
    if dense.dim() == 2:
        return dense.reshape(-1).to(dev())
    return widen(dense.reshape(P.n * P.L, -1), ld or dense.shape[2])


def untokens(P, t, cols=None):
    """The inverse, on the host: [n, L] / [n, L, cols] with 0 at the positions that do not exist."""
    t = t.detach().cpu()
    if P.packed:
        return R.unpack(t, P.rows, P.live, cols)
    return t.reshape(P.n, P.L) if t.dim() == 1 else t[:, :cols].reshape(P.n, P.L, cols)


def base_kw(P, S, mode=None):
    """The operands every call of the problem shares."""
    mode = mode or P.mode
    kw = dict(x=tokens(P, P.x, S['ldx']), ldx=S['ldx'], D=P.D, n=P.n, Lx=P.L, plan=P.plan)
    if P.mask is not None:
        kw.update(mask=P.mask.to(dev()), mask_div=P.mask_div)
    if mode == 'dot':
        kw.update(v=widen(P.v, S['ldv']), ldv=S['ldv'], scale=P.scale)
    return kw


def forward(P, S, kw, add_in=True, mode=None):
    from nnr_amd import ops
    mode = mode or P.mode
    alpha, out = Out(P.cap, 1), Out(P.n, P.D, S['ldo'])
    fk = dict(kw)
    if mode == 'given':
        fk.update(score=tokens(P, P.score))
    elif mode == 'th':
        fk.update(th=tokens(P, P.th, S['ldth'])[:, :P.A], w2=P.w2.to(dev()))
    if add_in:
        fk.update(add_in=widen(P.add_in, S['ldadd']), ldadd=S['ldadd'])
    ops.pool_fwd(alpha=alpha.full.view(-1), out=out.full, ldo=S['ldo'], **fk)
    alpha.check(P.live_rows, 'alpha')
    out.check(None, 'out')
    return alpha, out


def backward(P, S, kw, alpha, form, mode=None, fold=None):
    """One backward call in the given form; returns the Out buffers dx, dscore, dv (None where the form passes none)."""
    from nnr_amd import ops
    mode = mode or P.mode
    dot = mode == 'dot'
    bk = dict(kw, alpha=alpha.full.view(-1), dout=widen(P.dout, S['lddo']), lddo=S['lddo'])
    dx = dscore = dv = None
    if form in ('plain', 'acc', 'dout2', 'fold'):
        dx = Out(P.cap, P.D, S['lddx'], fill='pattern' if form == 'acc' else NAN)
        bk.update(dx=dx.full, lddx=S['lddx'], dx_accumulate=form == 'acc')
    if form in ('dout2', 'fold'):
        bk.update(dout2=widen(P.dout2, S['lddo2']), lddo2=S['lddo2'])
    if form != 'nothing':
        dscore = Out(P.cap, 1)
        bk.update(dscore=dscore.full.view(-1))
    if dot and form in ('plain', 'acc', 'dout2', 'dv_no_dx'):
        dv = Out(P.n, P.D, S['lddv'])
        bk.update(dv=dv.full, lddv=S['lddv'])
    if form == 'fold':
        bk.update(fold)
    ops.pool_bwd(**bk)
    for o, rows, what in ((dx, P.live_rows, 'dx'), (dscore, P.live_rows, 'dscore'), (dv, None, 'dv')):
        if o is not None:
            o.check(rows, '%s (%s)' % (what, form))
    return dx, dscore, dv


def check_all(P, ra, rb, S=None, tag=''):
    """Both forwards and every backward form of the problem against the references ra (upstream dout) and rb (dout + dout2).  Returns
    the bits of every output, for the determinism / stride comparisons."""
    S = S or strides(P)
    dot = P.mode == 'dot'
    kw = base_kw(P, S)
    bits = {}
    alpha, out = forward(P, S, kw, add_in=True)
    close(untokens(P, alpha.full.view(-1)), ra.alpha, what=tag + 'alpha')
    close(out.t, ra.out, what=tag + 'out + add_in')
    alpha0, out0 = forward(P, S, kw, add_in=False)
    close(out0.t, ra.out - P.add_in.double(), what=tag + 'out')
    assert same_bits(alpha0.full, alpha.full)
    bits.update(alpha=alpha.t.clone(), out=out.t.clone(), out0=out0.t.clone())
    for s in P.masked_seqs:                                          # a fully masked group: uniform over its tokens
        l = P.lens[s] if P.packed else P.L
        a = untokens(P, alpha.full.view(-1))[s, :l].double()
        assert float((a - 1.0 / l).abs().max()) <= 2e-5 / l, 'alpha of the fully masked sequence %d' % s

    def dense_dx(o, sub=None):
        t = o.full.detach().cpu().double()
        if sub is not None:
            t = t - sub.cpu().double()
        return untokens(P, t, P.D)

    for form in ('plain', 'acc', 'dout2', 'dscore_only', 'nothing') + (('dv_no_dx',) if dot else ()):
        dx, dscore, dv = backward(P, S, kw, alpha, form)
        r = rb if form == 'dout2' else ra
        t = '%s%s: ' % (tag, form)
        if dx is not None:
            # (acc: the pattern is taken off again, so the bar stays on the scale of dx itself, not on the pattern's)
            got = dense_dx(dx, dx.before[GUARD:GUARD + dx.rows * dx.ld].view(dx.rows, dx.ld) if form == 'acc' else None)
            close(got, r.dx, what=t + 'dx')
            bits[form + '.dx'] = dx.t.clone()
            for s in P.masked_seqs:
                l = P.lens[s] if P.packed else P.L
                g = (P.dout[s] + (P.dout2[s] if form == 'dout2' else 0.0)).double()
                close(got[s, :l], (1.0 / l) * g[None, :].expand(l, P.D), what=t + 'dx of the fully masked sequence %d' % s)
        if dscore is not None:
            ds = untokens(P, dscore.full.view(-1))
            close(ds, r.dscore, what=t + 'dscore')
            bits[form + '.dscore'] = dscore.t.clone()
            for s in P.masked_seqs:
                assert float(ds[s].abs().max()) == 0.0, 'dscore of the fully masked sequence %d is not exactly 0' % s
        if dv is not None:
            close(dv.t, r.dv, what=t + 'dv')
            bits[form + '.dv'] = dv.t.clone()
    return bits


def assert_same_outputs(b1, b2, what):
    assert b1.keys() == b2.keys()
    for k in b1:
        assert same_bits(b1[k], b2[k]), '%s: %s differs' % (what, k)


def refs(P):
    kw = dict(mask=P.mask, mask_div=P.mask_div, add_in=P.add_in)
    if P.mode == 'dot':
        kw.update(v=P.v, scale=P.scale)
    elif P.mode == 'th':
        kw.update(th=P.th, w2=P.w2)
    else:
        kw.update(score=P.score)
    return R.pool_ref(P.x, P.lens, dout=P.dout, **kw), R.pool_ref(P.x, P.lens, dout=P.dout, dout2=P.dout2, **kw)


@functools.lru_cache(maxsize=4)
def packed_problem(table, D, mode, A):
    L, lens = R.table_lens(table)
    P = problem(len(lens), L, D, lens, mode, A, seed=D + L)
    return (P,) + refs(P)


# ------------------------------------------------------------------------------------------------ packed, no mask
@pytest.mark.parametrize('table,D,mode,A,ldth', R.packed_cases())
def test_packed_pool_forward_and_every_backward_form(table, D, mode, A, ldth):
    P, ra, rb = packed_problem(table, D, mode, A)
    paths = {R.path_of(True, D, P.L, l) for l in P.lens}
    print('paths:', sorted(paths))
    S = strides(P, ldth=ldth)
    bits = check_all(P, ra, rb, S)
    if table == 'ladder' and D == 260:                               # the same launches again: the same bits
        assert_same_outputs(bits, check_all(P, ra, rb, S, tag='(second run) '), 'run to run')


# ------------------------------------------------------------------------------------------------ packed with the caller's hole mask
@pytest.mark.parametrize('L,D,mode', R.HOLE_CASES)
def test_packed_pool_with_a_hole_mask_over_the_cover_plan(L, D, mode):
    """functional.PackedAttentionFn: the plan is built from ops.mask_cover(mask), the pool applies the original mask to the scores, in the
    caller's row order (order[s] / mask_div).  Row 0 is fully masked: uniform alpha, dscore exactly 0, dx = alpha * dout."""
    mask = R.hole_mask(R.HOLE_N, L, L)
    lens = R.cover_lens(mask)
    P = problem(R.HOLE_N, L, D, lens, mode, R.TH_A if mode == 'th' else 0, mask=mask, seed=3 * L + D, plan_from_cover=True)
    assert P.masked_seqs == [0] and R.path_of(True, D, L, lens[0])[1] == {8: 'single', 20: 'team', 70: 'stream'}[L]
    ra, rb = refs(P)
    assert float((ra.alpha[0] - 1.0 / L).abs().max()) <= 1e-15 and float(ra.alpha[~mask & (torch.arange(R.HOLE_N) > 0)[:, None]].abs().max()) == 0.0
    check_all(P, ra, rb)


# ------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize('n,L,D,mode,mk', R.dense_cases())
def test_dense_pool_forward_and_every_backward_form(n, L, D, mode, mk):
    mask, div = None, 1
    if mk == 'div1':
        mask = R.hole_mask(n, L, n + L)
    elif mk == 'div3':
        mask, div = R.hole_mask(5, L, n + L)[[0, 4]].contiguous(), 3          # a fully masked row and one with holes, three sequences each
    P = problem(n, L, D, None, mode, R.TH_A if mode == 'th' else 0, mask=mask, mask_div=div, seed=n + D)
    assert mk == 'none' or P.masked_seqs == list(range(div))
    ra, rb = refs(P)
    check_all(P, ra, rb)


# ------------------------------------------------------------------------------------------------ two pools in one write
def fold_ref(P):
    return R.pool_ref(P.x, P.lens, score=P.score, mask=P.mask, mask_div=P.mask_div, dout=P.dout, dout2=P.dout2, v_b=P.v_b, scale_b=P.scale_b,
                      dout_b=P.dout_b)


def run_fold(P, S):
    """CNE's two pools over one token stream: the self pool (GIVEN score, upstream dout + dout2) and the cross pool (DOT with v_b,
    scale_b, upstream dout_b).  Two passes (store, then read-modify-write) and the one write; returns both sets of outputs."""
    kw = base_kw(P, S, mode='given')
    alpha_s, _ = forward(P, S, kw, add_in=False, mode='given')
    Pc = types.SimpleNamespace(**vars(P))
    Pc.v, Pc.scale, Pc.dout = P.v_b, P.scale_b, P.dout_b                  # the cross pool as a call of its own
    Sc = dict(S, ldv=S['ldv_b'], lddo=S['lddo_b'])
    kwc = dict(kw, v=widen(P.v_b, S['ldv_b']), ldv=S['ldv_b'], scale=P.scale_b)
    alpha_c, _ = forward(Pc, Sc, kwc, add_in=False, mode='dot')
    # two passes
    from nnr_amd import ops
    dx2, dv2, dsc2 = Out(P.cap, P.D, S['lddx']), Out(P.n, P.D, S['lddv']), Out(P.cap, 1)
    ops.pool_bwd(alpha=alpha_c.full.view(-1), dout=widen(P.dout_b, S['lddo_b']), lddo=S['lddo_b'], dx=dx2.full, lddx=S['lddx'], dv=dv2.full,
                 lddv=S['lddv'], dscore=dsc2.full.view(-1), **kwc)
    ds2 = Out(P.cap, 1)
    ops.pool_bwd(alpha=alpha_s.full.view(-1), dout=widen(P.dout, S['lddo']), lddo=S['lddo'], dout2=widen(P.dout2, S['lddo2']), lddo2=S['lddo2'],
                 dx=dx2.full, lddx=S['lddx'], dx_accumulate=True, dscore=ds2.full.view(-1), **kw)
    for o, rows in ((dx2, P.live_rows), (dv2, None), (dsc2, P.live_rows), (ds2, P.live_rows)):
        o.check(rows, 'two passes')
    # one write: the cross pool leaves dscore and dv (dx = NULL), the self pool's backward folds its token gradient in
    _, ds_c, dv1 = backward(Pc, Sc, kwc, alpha_c, 'dv_no_dx', mode='dot')
    fold = dict(alpha_b=alpha_c.full.view(-1), dout_b=widen(P.dout_b, S['lddo_b']), lddo_b=S['lddo_b'], dscore_b=ds_c.full.view(-1),
                v_b=widen(P.v_b, S['ldv_b']), ldv_b=S['ldv_b'], scale_b=P.scale_b)
    dx1, ds1, _ = backward(P, S, kw, alpha_s, 'fold', mode='given', fold=fold)
    return types.SimpleNamespace(dx1=dx1, ds1=ds1, ds_c=ds_c, dv1=dv1, dx2=dx2, dv2=dv2, dsc2=dsc2, ds2=ds2, alpha_s=alpha_s, alpha_c=alpha_c)


def check_fold(P, r, o, tag=''):
    close(untokens(P, o.alpha_s.full.view(-1)), r.alpha, what=tag + 'fold alpha (self)')
    close(untokens(P, o.alpha_c.full.view(-1)), r.alpha_b, what=tag + 'fold alpha (cross)')
    close(untokens(P, o.dx1.full, P.D), r.dx, what=tag + 'two pools, one write: dx')
    close(o.dv1.t, r.dv_b, what=tag + 'two pools: dv')
    close(untokens(P, o.ds1.full.view(-1)), r.dscore, what=tag + 'two pools: dscore (self)')
    close(untokens(P, o.ds_c.full.view(-1)), r.dscore_b, what=tag + 'two pools: dscore (cross)')
    assert same_bits(o.dv1.t, o.dv2.t) and same_bits(o.ds1.full, o.ds2.full) and same_bits(o.ds_c.full, o.dsc2.full)
    a, b = untokens(P, o.dx1.full, P.D), untokens(P, o.dx2.full, P.D)
    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())      # same terms, possibly another fma contraction


@functools.lru_cache(maxsize=2)
def fold_problem(table, D):
    if table == 'dense':
        n, L, D = R.STRIDE_DENSE
        P = problem(n, L, D, None, 'given', seed=77)
    else:
        L, lens = R.table_lens(table)
        P = problem(len(lens), L, D, lens, 'given', seed=D + L + 1)
    return P, fold_ref(P)


@pytest.mark.parametrize('table,D', R.FOLD_CASES)
def test_backward_of_two_pools_in_one_write(table, D):
    P, r = fold_problem(table, D)
    check_fold(P, r, run_fold(P, strides(P)))


# ------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize('table,D', R.STRIDE_CASES)
def test_every_leading_dimension_wider_than_the_row(table, D):
    """ldx, ldv, ldo, ldadd, lddo, lddo2, lddx, lddv, lddo_b, ldv_b and ldth all distinct and greater than the row: the results are the
    compact call's, bit for bit, and the gap columns keep their bits (Out.check inside every call)."""
    A = R.TH_A
    for mode in ('dot', 'th'):
        if table == 'dense':
            n, L, D = R.STRIDE_DENSE
            P = problem(n, L, D, None, mode, A if mode == 'th' else 0, seed=5)
            ra, rb = refs(P)
        else:
            P, ra, rb = packed_problem(table, D, mode, A if mode == 'th' else 0)
        wide = wide_strides(P)
        assert all(v % 4 == 0 and v > (P.A if k == 'ldth' else P.D) for k, v in wide.items() if v)
        assert_same_outputs(check_all(P, ra, rb, wide, tag='(wide) '), check_all(P, ra, rb), 'wide against compact')
    P, r = fold_problem(table, D)
    ow, oc = run_fold(P, wide_strides(P)), run_fold(P, strides(P))
    check_fold(P, r, ow, tag='(wide) ')
    for k in ('dx1', 'ds1', 'ds_c', 'dv1', 'dx2', 'dv2'):
        assert same_bits(getattr(ow, k).t, getattr(oc, k).t), 'fold, wide against compact: %s differs' % k


# ------------------------------------------------------------------------------------------------ refusals
def test_pool_refuses_what_it_cannot_run():
    """Return codes only: nothing is launched, every output keeps its NaNs.  -3 = NNR_ERR_UNSUPPORTED, -1 = NNR_ERR_ARG."""
    from nnr_amd import ops
    from nnr_amd._lib import NnrHipError
    d = dev()
    outs = []

    def nan(*shape):
        t = torch.full(shape, NAN, device=d)
        outs.append(t)
        return t

    def zeros(*shape):
        return torch.zeros(shape, device=d)

    def refused(code, fn, **kw):
        with pytest.raises(NnrHipError) as e:
            fn(**kw)
        assert str(e.value).endswith('code %d' % code), str(e.value)

    def fwd_kw(n, L, D, ldx=None):
        ldx = ldx or D
        return dict(x=zeros(n * L, ldx), ldx=ldx, D=D, n=n, Lx=L, score=zeros(n * L), alpha=nan(n * L), out=nan(n, D + 4), ldo=D + 4)

    n, L, D = 2, 5, 8
    refused(-3, ops.pool_fwd, **fwd_kw(n, L, 1284))
    refused(-3, ops.pool_fwd, **fwd_kw(n, L, 6))
    refused(-3, ops.pool_fwd, **fwd_kw(n, 129, D))
    refused(-3, ops.pool_fwd, **fwd_kw(n, L, D, ldx=D + 2))
    kw = fwd_kw(n, L, D)
    kw.pop('score')
    refused(-3, ops.pool_fwd, th=zeros(n * L, 260), w2=zeros(260), **kw)                    # A > 256
    refused(-3, ops.pool_fwd, th=zeros(n * L, 10)[:, :6], w2=zeros(8), **kw)                # A % 4
    refused(-3, ops.pool_fwd, th=zeros(n * L, 10)[:, :8], w2=zeros(8), **kw)                # ldth % 4
    # every operand the kernels move as float4: a pointer that is set with a leading dimension that is no multiple of 4
    odd = D + 2
    wide = lambda rows: zeros(rows, D + 4)                                                   # noqa: E731
    base = dict(x=zeros(n * L, D), ldx=D, D=D, n=n, Lx=L)
    f = dict(base, score=zeros(n * L), alpha=nan(n * L))
    refused(-3, ops.pool_fwd, out=nan(n, D + 4), ldo=odd, **f)
    refused(-3, ops.pool_fwd, out=nan(n, D + 4), ldo=D + 4, add_in=wide(n), ldadd=odd, **f)
    f.pop('score')
    refused(-3, ops.pool_fwd, out=nan(n, D + 4), ldo=D + 4, v=wide(n), ldv=odd, scale=1.0, **f)
    b = dict(base, alpha=zeros(n * L), dout=wide(n), lddo=D + 4)
    refused(-3, ops.pool_bwd, **dict(b, lddo=odd))
    refused(-3, ops.pool_bwd, dout2=wide(n), lddo2=odd, dscore=nan(n * L), **b)
    refused(-3, ops.pool_bwd, dx=nan(n * L, D + 4), lddx=odd, **b)
    refused(-3, ops.pool_bwd, v=wide(n), ldv=D + 4, scale=1.0, dv=nan(n, D + 4), lddv=odd, **b)
    refused(-3, ops.pool_bwd, v=wide(n), ldv=odd, scale=1.0, dv=nan(n, D + 4), lddv=D + 4, **b)
    fold = dict(alpha_b=zeros(n * L), dout_b=wide(n), lddo_b=D + 4, dscore_b=zeros(n * L), v_b=wide(n), ldv_b=D + 4, scale_b=1.0)
    refused(-3, ops.pool_bwd, dx=nan(n * L, D + 4), lddx=D + 4, **dict(fold, lddo_b=odd), **b)
    refused(-3, ops.pool_bwd, dx=nan(n * L, D + 4), lddx=D + 4, **dict(fold, ldv_b=odd), **b)
    # incomplete second-pool arguments, a second pool on top of an accumulating dx, no out, no alpha
    for missing in ('dout_b', 'dscore_b', 'v_b'):
        part = dict(fold)
        part.pop(missing)
        refused(-1, ops.pool_bwd, dx=nan(n * L, D + 4), lddx=D + 4, **part, **b)
    refused(-1, ops.pool_bwd, **fold, **b)                                                   # the fold is a write of dx
    refused(-1, ops.pool_bwd, dx=nan(n * L, D + 4), lddx=D + 4, dx_accumulate=True, **fold, **b)
    refused(-1, ops.pool_fwd, score=zeros(n * L), alpha=nan(n * L), **base)
    nb = dict(b)
    nb.pop('alpha')
    refused(-1, ops.pool_bwd, dx=nan(n * L, D + 4), lddx=D + 4, **nb)
    refused(-1, ops.pool_bwd, score=zeros(n * L), dx=nan(n * L, D + 4), lddx=D + 4, **nb)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), 'a refused call wrote to an output'
