"""Every kernel instantiation behind the MHSA attention core's eight entry points (csrc/mhsa.hip: dense, packed rows, paired short titles,
forward and backward) against the float64 restatement of tests/mhsa_ref.py, under the project's 2e-5 bar taken per (sample, head, matrix)
slice.  Each case also pins the fused dropout to ops.dropout bit for bit, a second call to the same bits, and NaN guard rows around (and,
for packed buffers, behind) the rows the kernels own.  Shapes, masks and inputs come from mhsa_ref, where tests/test_mhsa_host.py checks on
the CPU that they reach what they claim (group plans, pair layouts, all twelve instantiations, no degenerate slice)."""
import pytest
import torch

import mhsa_ref as R

pytestmark = pytest.mark.gpu

GUARD = 8          # NaN rows in front of and behind every output


def dev():
    return torch.device('cuda:0')


def guarded(rows, cols):
    big = torch.full((rows + 2 * GUARD, cols), float('nan'), device=dev())
    return big, big[GUARD:GUARD + rows]


def untouched(big, rows, total, what):
    """The guard rows, and the rows >= total of a packed buffer, still hold NaN; the rows below total hold numbers."""
    assert bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[GUARD + rows:]).all()), '%s: a guard row was written' % what
    assert bool(torch.isnan(big[GUARD + total:GUARD + rows]).all()), '%s: a row beyond the live count was written' % what
    assert bool(torch.isfinite(big[GUARD:GUARD + total]).all()), '%s: a live row holds a NaN / Inf' % what


def check_core(case, fwd, bwd, rows, total, dout_dev, to_dense=lambda t: t, live=None):
    """fwd(out, p, seed) / bwd(dout, dqkv, p, seed) run one entry point over buffers of `rows` rows of which `total` are live."""
    from nnr_amd import ops
    n, Lq, heads, dh = case.n, case.Lq, case.heads, case.dh
    HD = heads * dh
    ref_out, ref_dqkv = R.reference(case)
    p, seed = R.DROP
    # ---- forward
    big, out = guarded(rows, HD)
    fwd(out, 0.0, 0)
    untouched(big, rows, total, case.tag + ' out')
    worst_o = R.slice_bar(to_dense(out), ref_out, n, Lq, heads, dh, 1, live, what=case.tag + ' out')
    big2, out2 = guarded(rows, HD)
    fwd(out2, 0.0, 0)
    assert torch.equal(out2[:total], out[:total]), '%s: the forward is not deterministic' % case.tag
    bigp, outp = guarded(rows, HD)
    fwd(outp, p, seed)
    untouched(bigp, rows, total, case.tag + ' out (dropout)')
    assert torch.equal(outp[:total], ops.dropout(out, p, seed)[:total]), '%s: fused dropout (forward)' % case.tag
    # ---- backward
    bigd, dq = guarded(rows, 3 * HD)
    bwd(dout_dev, dq, 0.0, 0)
    untouched(bigd, rows, total, case.tag + ' dqkv')
    worst_g = R.slice_bar(to_dense(dq), ref_dqkv, n, Lq, heads, dh, 3, live, what=case.tag + ' dqkv')
    bigd2, dq2 = guarded(rows, 3 * HD)
    bwd(dout_dev, dq2, 0.0, 0)
    assert torch.equal(dq2[:total], dq[:total]), '%s: the backward is not deterministic' % case.tag
    bigf, dqf = guarded(rows, 3 * HD)
    bwd(dout_dev, dqf, p, seed)
    untouched(bigf, rows, total, case.tag + ' dqkv (dropout)')
    bigs, dqs = guarded(rows, 3 * HD)
    bwd(ops.dropout(dout_dev, p, seed), dqs, 0.0, 0)
    assert torch.equal(dqf[:total], dqs[:total]), '%s: fused dropout (backward)' % case.tag
    print('PARITY %s: out %.3f dqkv %.3f of the per-slice bar' % (case.tag, worst_o, worst_g))


# ------------------------------------------------------------------------------------------------ a. dense
def run_dense(case, saved_prob):
    from nnr_amd import ops
    d = dev()
    n, Lq, heads, dh = case.n, case.Lq, case.heads, case.dh
    (f, cf), (b, cb) = R.dispatch(Lq, heads, dh, saved_prob)
    print('KERNELS %s prob=%d: %s coop=%d, %s coop=%d' % (case.tag, saved_prob, f, cf, b, cb))
    qd = case.qkv.to(d)
    md = None if case.mask is None else case.mask.to(d)
    prob = torch.empty(ops.mhsa_prob_size(n, Lq, heads), device=d) if saved_prob else None
    check_core(case,
               lambda out, p, seed: ops.mhsa_fwd(qd, md, n, Lq, heads, dh, out, prob, p, seed),
               lambda dout, dq, p, seed: ops.mhsa_bwd(qd, md, prob, dout, n, Lq, heads, dh, dq, p, seed),
               n * Lq, n * Lq, case.dout.to(d))


@pytest.mark.parametrize('kind', R.DENSE_KINDS)
@pytest.mark.parametrize('saved_prob', [True, False])
@pytest.mark.parametrize('n,Lq,heads,dh', R.DENSE_SHAPES)
def test_mhsa_dense_matches_fp64_per_slice(n, Lq, heads, dh, saved_prob, kind):
    run_dense(R.dense_case(n, Lq, heads, dh, kind), saved_prob)


@pytest.mark.parametrize('n,Lq,heads,dh', R.GROUP_LOOP_SHAPES)
def test_mhsa_persistent_backward_walks_several_groups(n, Lq, heads, dh):
    """gp > 1: the prefetch of the next group's tiles, the per-group key-mask byte, workgroups that straddle two samples and a ragged last
    workgroup (heads = 12), or exactly one sample's groups each (heads = 8)."""
    ngroups, gp = R.group_plan(heads, n)
    assert gp == 2 and ngroups == n * heads // 4 >= 2048
    assert R.dispatch(Lq, heads, dh, False)[1][0].startswith('persist')
    run_dense(R.group_loop_case(n, Lq, heads, dh), False)


# ------------------------------------------------------------------------------------------------ b / c. packed rows, paired titles
class Packed:
    """The case's plan, row map and packed buffers (rows that do not exist hold NaN)."""

    def __init__(self, case):
        from nnr_amd import ops
        d = dev()
        n, L = case.n, case.Lq
        self.md = case.mask.to(d)
        cover = ops.mask_cover(self.md)
        assert torch.equal(cover.cpu().bool(), case.cover), '%s: mask_cover' % case.tag
        self.plan = ops.SeqPlan(cover, None)
        self.rowmap = ops.seq_rowmap(self.plan)
        self.rm = self.rowmap.cpu().view(n, L).long()
        self.total = int(self.plan.total.item())
        assert torch.equal(self.rm >= 0, case.cover) and self.total == int(case.cover.sum())
        self.rows = self.rm[case.cover]                                              # packed row of every live position, in dense order
        assert sorted(self.rows.tolist()) == list(range(self.total)), '%s: the row map is no bijection onto the packed rows' % case.tag
        self.cap = self.plan.cap
        self.live = case.cover
        self.qp = self.pack(case.qkv)
        self.dp = self.pack(case.dout)

    def pack(self, dense):
        buf = torch.full((self.cap, dense.shape[1]), float('nan'))
        buf[self.rows] = dense[self.live.reshape(-1)]
        return buf.to(dev())

    def to_dense(self, buf):
        out = torch.zeros((self.live.numel(), buf.shape[1]), dtype=buf.dtype)
        out[self.live.reshape(-1)] = buf.detach().cpu()[self.rows]
        return out


@pytest.mark.parametrize('profile', R.PACKED_PROFILES)
@pytest.mark.parametrize('n,L,heads,dh', R.PACKED_SHAPES)
def test_mhsa_packed_rows_match_fp64_per_slice(n, L, heads, dh, profile):
    from nnr_amd import ops
    case = R.packed_case(n, L, heads, dh, profile)
    pk = Packed(case)
    (f, cf), (b, cb) = R.dispatch(L, heads, dh, False)
    print('KERNELS %s: %s coop=%d, %s coop=%d, packed' % (case.tag, f, cf, b, cb))
    check_core(case,
               lambda out, p, seed: ops.mhsa_fwd_packed(pk.qp, pk.md, pk.rowmap, pk.plan, heads, dh, out, p, seed),
               lambda dout, dq, p, seed: ops.mhsa_bwd_packed(pk.qp, pk.md, pk.rowmap, pk.plan, dout, heads, dh, dq, p, seed),
               pk.cap, pk.total, pk.dp, pk.to_dense, pk.live)


def run_paired(case):
    from nnr_amd import ops
    heads, dh = case.heads, case.dh
    pk = Packed(case)
    plan = pk.plan
    pair = ops.mhsa_pair_map(plan, pk.md)
    # the maps, before any attention kernel runs
    slen, off, order = plan.slen.cpu(), plan.off.cpu(), plan.order.cpu()
    lay = R.pair_layout(slen)
    assert (lay.n16, lay.n8) == (int(off[17] - off[16]), int(off[9] - off[8]))
    want_row, want_mask = R.pair_maps(lay, off, slen, order, case.mask)
    vrow, vmask = pair[0].cpu(), pair[1].cpu()
    placed = vrow[:lay.nv][vrow[:lay.nv] >= 0]
    assert sorted(placed.tolist()) == list(range(pk.total)), '%s: a packed row is missing or placed twice' % case.tag
    assert bool((vrow[lay.nv:] == -1).all()) and bool((vmask[lay.nv:] == 0).all())
    assert torch.equal(vrow, want_row), '%s: vrowmap differs from pair_layout' % case.tag
    assert torch.equal(vmask, want_mask), '%s: vmask is not the original mask of the placed positions' % case.tag
    (f, cf), (b, cb) = R.dispatch(32, heads, dh, False)
    print('KERNELS %s: %s coop=%d, %s coop=%d, paired (n16 %d, pairs %d, nv %d of n %d)' % (case.tag, f, cf, b, cb, lay.n16, lay.np, lay.nv, case.n))
    check_core(case,
               lambda out, p, seed: ops.mhsa_fwd_paired(pk.qp, pair, plan, heads, dh, out, p, seed),
               lambda dout, dq, p, seed: ops.mhsa_bwd_paired(pk.qp, pair, plan, dout, heads, dh, dq, p, seed),
               pk.cap, pk.total, pk.dp, pk.to_dense, pk.live)


@pytest.mark.parametrize('profile', R.PAIRED_PROFILES)
@pytest.mark.parametrize('dh', R.PAIRED_DHS)
def test_mhsa_paired_titles_match_fp64_per_title(dh, profile):
    run_paired(R.paired_case(profile, 4, dh))


def test_mhsa_paired_titles_with_several_groups_per_workgroup():
    """gp > 1 on the paired path: the persistent backward's group count follows nv (virtual samples) while its grid follows n."""
    profile, n, heads, dh = R.PAIRED_GROUP_LOOP
    assert R.group_plan(heads, n)[1] > 1
    run_paired(R.paired_case(profile, heads, dh, n))


# ------------------------------------------------------------------------------------------------ d. what the entry points refuse
def _nan(rows, cols):
    return torch.full((rows, cols), float('nan'), device=dev())


def _still_nan(*bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b).all()) for b in bufs)


@pytest.mark.parametrize('n,Lq,heads,dh', [(2, 65, 4, 20), (2, 32, 4, 34), (2, 32, 4, 5)])
def test_mhsa_dense_refuses_what_it_cannot_tile(n, Lq, heads, dh):
    from nnr_amd import ops
    from nnr_amd._lib import NnrHipError
    HD = heads * dh
    qkv = torch.zeros(n * Lq, 3 * HD, device=dev())
    mask = torch.ones(n, Lq, dtype=torch.bool, device=dev())
    out, dq = _nan(n * Lq, HD), _nan(n * Lq, 3 * HD)
    with pytest.raises(NnrHipError):
        ops.mhsa_fwd(qkv, mask, n, Lq, heads, dh, out, None)
    with pytest.raises(NnrHipError):
        ops.mhsa_bwd(qkv, mask, None, torch.zeros(n * Lq, HD, device=dev()), n, Lq, heads, dh, dq)
    assert _still_nan(out, dq)


def _plan_for(n, L):
    from nnr_amd import ops
    mask = R._prefix(torch.randint(1, L + 1, (n,), generator=torch.Generator().manual_seed(9)), L).to(dev())
    plan = ops.SeqPlan(ops.mask_cover(mask), None)
    return mask, plan, ops.seq_rowmap(plan)


@pytest.mark.parametrize('heads,dh', [(5, 20), (4, 6)])
def test_mhsa_packed_refuses_the_one_head_per_wave_shapes(heads, dh):
    from nnr_amd import ops
    from nnr_amd._lib import NnrHipError
    HD = heads * dh
    mask, plan, rowmap = _plan_for(12, 32)
    qkv = torch.zeros(plan.cap, 3 * HD, device=dev())
    out, dq = _nan(plan.cap, HD), _nan(plan.cap, 3 * HD)
    with pytest.raises(NnrHipError):
        ops.mhsa_fwd_packed(qkv, mask, rowmap, plan, heads, dh, out)
    with pytest.raises(NnrHipError):
        ops.mhsa_bwd_packed(qkv, mask, rowmap, plan, torch.zeros(plan.cap, HD, device=dev()), heads, dh, dq)
    assert _still_nan(out, dq)


def test_mhsa_paired_refuses_other_lengths_and_the_backward_a_wide_head():
    from nnr_amd import ops
    from nnr_amd._lib import NnrHipError
    mask20, plan20, _ = _plan_for(12, 20)
    with pytest.raises(NnrHipError):
        ops.mhsa_pair_map(plan20, mask20)
    heads, dh = 4, 28                        # 32 * dh > 768: the persistent kernel, the only paired backward, does not hold it
    HD = heads * dh
    mask, plan, _ = _plan_for(12, 32)
    pair = ops.mhsa_pair_map(plan, mask)
    dq = _nan(plan.cap, 3 * HD)
    with pytest.raises(NnrHipError):
        ops.mhsa_bwd_paired(torch.zeros(plan.cap, 3 * HD, device=dev()), pair, plan, torch.zeros(plan.cap, HD, device=dev()), heads, dh, dq)
    assert _still_nan(dq)


def test_packed_core_function_keeps_both_directions_on_the_packed_kernels_at_dh_28(monkeypatch):
    """The paired forward would accept heads = 4, dh = 28; the paired backward refuses it.  functional.PackedMhsaCoreFn's chooser is what
    keeps the two directions on the same kernels: both must take the packed (row-mapped) ones, and match float64."""
    from nnr_amd import functional as F, ops
    n, L, heads, dh = 40, 32, 4, 28
    case = R.packed_case(n, L, heads, dh, 'edges')
    pk = Packed(case)
    pack = F.MhsaPack(pk.md, torch.zeros((n, L), dtype=torch.int32, device=dev()))
    assert pack.pair is not None and torch.equal(pack.rowmap, pk.rowmap)
    calls = []
    for name in ('mhsa_fwd_packed', 'mhsa_bwd_packed', 'mhsa_fwd_paired', 'mhsa_bwd_paired'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    x = pk.qp.clone().requires_grad_(True)
    out = F.PackedMhsaCoreFn.apply(x, pk.md, pack, heads, dh, 0.0, 0)
    out.backward(pk.dp)
    assert calls == ['mhsa_fwd_packed', 'mhsa_bwd_packed'], calls
    ref_out, ref_dqkv = R.reference(case)
    R.slice_bar(pk.to_dense(out), ref_out, n, L, heads, dh, 1, pk.live, what='PackedMhsaCoreFn out')
    R.slice_bar(pk.to_dense(x.grad), ref_dqkv, n, L, heads, dh, 3, pk.live, what='PackedMhsaCoreFn dqkv')
