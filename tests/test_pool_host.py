"""CPU checks of what tests/test_hip_pool_gpu.py stands on: the float64 restatement of the attention pool (tests/pool_ref.py) against the
oracle's AdditivePool and CandidatePool, its behaviour on a fully masked row, the packing helpers, and the coverage of the kernel's paths
(csrc/pool.hip: instantiation x body, the length boundaries, the fill of the last single-wave workgroup) by the shared case tables."""
import math

import pytest
import torch

import pool_ref as R


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _err(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize('masked', [False, True])
def test_pool_ref_equals_the_oracles_additive_pool(masked):
    from oracle.nnr_oracle import AdditivePool
    torch.manual_seed(1)
    n, L, F, A = 7, 11, 12, 8
    ref = AdditivePool(F, A).double()
    ref.initialize()
    with torch.no_grad():
        ref.affine1.bias.normal_(0, 0.1)
    x, dout = _randn((n, L, F), 2), _randn((n, F), 3)
    mask = R.hole_mask(n, L, 4) if masked else None
    xr = x.clone().requires_grad_(True)
    want = ref(xr, mask)
    want.backward(dout)
    th = torch.tanh(ref.affine1(x)).detach()
    w2 = ref.affine2.weight.detach()[0]
    for kw in (dict(th=th, w2=w2), dict(score=th @ w2)):
        r = R.pool_ref(x, mask=mask, dout=dout, **kw)
        assert r.out.dtype == torch.float64 and _err(r.out, want.detach()) <= 1e-12
        # d x of the layer = the pool's own dx + dscore carried through w2 . tanh(W1 x + b1)
        x2 = x.clone().requires_grad_(True)
        (torch.tanh(ref.affine1(x2)) @ w2).backward(r.dscore)
        assert _err(r.dx + x2.grad, xr.grad) <= 1e-12
        assert r.dv is None


@pytest.mark.parametrize('masked', [False, True])
def test_pool_ref_equals_the_oracles_candidate_pool(masked):
    from oracle.nnr_oracle import CandidatePool
    torch.manual_seed(5)
    n, L, F, Q, A = 6, 9, 12, 10, 8
    ref = CandidatePool(F, Q, A).double()
    ref.initialize()
    with torch.no_grad():
        ref.Q.bias.normal_(0, 0.1)
    x, q, dout = _randn((n, L, F), 6), _randn((n, Q), 7), _randn((n, F), 8)
    mask = R.hole_mask(n, L, 9) if masked else None
    xr, qr = x.clone().requires_grad_(True), q.clone().requires_grad_(True)
    want = ref(xr, qr, mask)
    want.backward(dout)
    v = (ref.Q(q) @ ref.K.weight).detach()                  # K^T (Q q + b): the GEMV form of (K x) . (Q q)
    r = R.pool_ref(x, v=v, scale=1.0 / math.sqrt(A), mask=mask, dout=dout)
    assert _err(r.out, want.detach()) <= 1e-12
    assert _err(r.dx, xr.grad) <= 1e-12
    q2 = q.clone().requires_grad_(True)
    (ref.Q(q2) @ ref.K.weight).backward(r.dv)
    assert _err(q2.grad, qr.grad) <= 1e-12


def test_pool_ref_lengths_mask_groups_second_pool_and_add_in():
    """lens = softmax over t < len (the rest of the row may hold anything finite), mask_div shares a mask row, the second pool adds its
    token gradient, add_in is added to out only."""
    n, L, D = 6, 7, 8
    x, sc, v, dout, dout_b, add = _randn((n, L, D), 1), _randn((n, L), 2), _randn((n, D), 3, 0.3), _randn((n, D), 4), _randn((n, D), 5), _randn((n, D), 6)
    lens = [7, 1, 4, 2, 7, 3]
    mask = R.hole_mask(2, L, 7)
    r = R.pool_ref(x, lens, score=sc, mask=mask, mask_div=3, add_in=add, dout=dout, v_b=v, scale_b=0.4, dout_b=dout_b)
    a = R.pool_ref(x, lens, score=sc, mask=mask, mask_div=3, dout=dout)
    b = R.pool_ref(x, lens, v=v, scale=0.4, mask=mask, mask_div=3, dout=dout_b)
    assert _err(r.dx, a.dx + b.dx) <= 1e-14 and _err(r.dscore_b, b.dscore) == 0.0 and _err(r.dv_b, b.dv) == 0.0 and _err(r.alpha_b, b.alpha) == 0.0
    assert _err(r.out, a.out + add) == 0.0
    for i, l in enumerate(lens):
        keep = mask[i // 3, :l]
        s = torch.where(keep, sc[i, :l], torch.full((l,), -1e9, dtype=torch.float64))
        al = torch.softmax(s, 0)
        assert _err(a.alpha[i, :l], al) <= 1e-15 and float(a.alpha[i, l:].abs().sum()) == 0.0
        assert _err(a.out[i], al @ x[i, :l]) <= 1e-14
        assert float(a.dx[i, l:].abs().sum()) == 0.0 and float(a.dscore[i, l:].abs().sum()) == 0.0


def test_pool_ref_on_a_fully_masked_row_is_uniform_with_no_score_gradient():
    n, L, D = 4, 10, 8
    x, sc, v, dout = _randn((n, L, D), 1), _randn((n, L), 2), _randn((n, D), 3), _randn((n, D), 4)
    mask = R.hole_mask(n, L, 5)
    assert not bool(mask[0].any())
    for kw in (dict(score=sc), dict(v=v, scale=0.5)):
        r = R.pool_ref(x, mask=mask, dout=dout, **kw)
        assert float((r.alpha[0] - 1.0 / L).abs().max()) <= 1e-15
        assert float(r.dscore[0].abs().max()) == 0.0
        assert _err(r.dx[0], r.alpha[0][:, None] * dout[0][None, :]) <= 1e-15
        assert float(r.dscore[1].abs().max()) > 0.0
    # with lengths (the packed form of a fully masked title: all L positions, functional.MhsaPack) and a shorter fully masked prefix
    r = R.pool_ref(x, [L, 3, L, 1], score=sc, mask=torch.zeros(n, L, dtype=torch.bool), dout=dout)
    assert float((r.alpha[1, :3] - 1.0 / 3).abs().max()) <= 1e-15 and float(r.alpha[1, 3:].abs().max()) == 0.0
    assert float(r.dscore.abs().max()) == 0.0


def test_hole_mask_rows_and_cover_lengths():
    m = R.hole_mask(R.HOLE_N, 20, 3)
    assert not m[0].any() and m[1].all() and m[2].nonzero().flatten().tolist() == [19] and m[3].nonzero().flatten().tolist() == [0]
    assert all(bool(m[i].any()) and not bool(m[i].all()) for i in range(4, R.HOLE_N))
    lens = R.cover_lens(m)
    assert lens[:4] == [20, 20, 20, 1]
    for i in range(4, R.HOLE_N):
        assert lens[i] == int(m[i].nonzero().max()) + 1
    assert R.cover_lens(R.hole_mask(3, 1, 0)) == [1, 1, 1]


def test_pack_and_unpack_are_inverse_and_fill_the_rest():
    L, lens = R.table_lens('mid')
    n = len(lens)
    lt = torch.tensor(lens)
    order = sorted(range(n), key=lambda i: -lens[i])                 # stable descending: nnr_seq_plan
    rank = torch.empty(n, dtype=torch.long)
    rank[torch.tensor(order)] = torch.arange(n)
    bs = [(lt > t).sum().item() for t in range(L)]
    off = torch.tensor([sum(bs[:t]) for t in range(L + 1)])
    rows = R.packed_rows(off, rank, L)
    live = torch.arange(L)[None, :] < lt[:, None]
    total = int(off[L])
    assert sorted(rows[live].tolist()) == list(range(total))         # the live positions fill the leading rows, each once
    x = _randn((n, L, 4), 1)
    xp = R.pack(x, rows, live, n * L, ld=6)
    assert xp.shape == (n * L, 6) and bool(torch.isnan(xp[total:]).all()) and bool(torch.isnan(xp[:, 4:]).all())
    assert not bool(torch.isnan(xp[:total, :4]).any())
    back = R.unpack(xp, rows, live, 4)
    assert torch.equal(back[live], x[live]) and float(back[~live].abs().sum()) == 0.0
    sp = R.pack(x[..., 0], rows, live, n * L)
    assert torch.equal(R.unpack(sp, rows, live)[live], x[..., 0][live])


# ------------------------------------------------------------------------------------------------ coverage of the kernel's paths
def test_path_of_follows_the_dispatch():
    assert R.path_of(True, 256, 128, 8) == ('packed NV1', 'single') and R.path_of(True, 256, 128, 9) == ('packed NV1', 'team')
    assert R.path_of(True, 260, 128, 32) == ('packed NV2', 'team') and R.path_of(True, 512, 128, 33) == ('packed NV2', 'stream')
    assert R.path_of(True, 260, 8, 8) == ('packed NV2', 'single') and R.path_of(True, 260, 32, 32) == ('packed NV2', 'team')
    assert R.path_of(True, 516, 128, 1) == ('pool_kernel NV4', 'stream') and R.path_of(True, 1280, 128, 1) == ('pool_kernel NV5', 'stream')
    assert R.path_of(False, 4, 1, 1) == ('pool_kernel NV1', 'stream') and R.path_of(False, 256, 64, 64) == ('pool_kernel NV1', 'stream')
    assert R.path_of(False, 260, 65, 65) == ('pool_kernel NV2', 'stream') and R.path_of(False, 512, 9, 9) == ('pool_kernel NV2', 'stream')
    assert R.path_of(False, 1024, 9, 9) == ('pool_kernel NV4', 'stream') and R.path_of(False, 1028, 9, 9) == ('pool_kernel NV5', 'stream')


def _packed_paths():
    """(instantiation, body, mode) over every sequence of every packed case."""
    out = set()
    for (table, D, mode, A, ldth) in R.packed_cases():
        L, lens = R.table_lens(table)
        out |= {R.path_of(True, D, L, l) + (mode,) for l in lens}
    return out


def test_case_tables_reach_every_instantiation_and_body_in_every_mode():
    existing = {(i, b) for i in ('packed NV1', 'packed NV2') for b in R.BODIES} | {(i, 'stream') for i in R.INSTANTIATIONS if i.startswith('pool_kernel')}
    packed = _packed_paths()
    dense = {R.path_of(False, D, L, L) + (m,) for (n, L, D, m, mk) in R.dense_cases()}
    assert {p[:2] for p in packed | dense} == existing
    for mode in R.MODES:                                             # every body of the packed kernels and the packed pool_kernel, in every mode
        for i in ('packed NV1', 'packed NV2'):
            for b in R.BODIES:
                assert (i, b, mode) in packed, (i, b, mode)
        assert ('pool_kernel NV4', 'stream', mode) in packed and ('pool_kernel NV5', 'stream', mode) in packed
    for mode in ('given', 'dot'):
        assert {i for (i, b, m) in dense if m == mode} == {i for i in R.INSTANTIATIONS if i.startswith('pool_kernel')}
    assert {i for (i, b, m) in dense if m == 'th'} >= {'pool_kernel NV1', 'pool_kernel NV2'}
    # the fold, the strides and the hole masks: every body of the packed kernels and pool_kernel
    fold = {R.path_of(True, D, R.table_lens(t)[0], l) for (t, D) in R.FOLD_CASES for l in R.table_lens(t)[1]}
    assert fold >= {(i, b) for i in ('packed NV1', 'packed NV2') for b in R.BODIES} | {('pool_kernel NV4', 'stream')}
    strides = set()
    for (t, D) in R.STRIDE_CASES:
        if t == 'dense':
            strides.add(R.path_of(False, R.STRIDE_DENSE[2], R.STRIDE_DENSE[1], R.STRIDE_DENSE[1])[0])
        else:
            strides |= {R.path_of(True, D, R.table_lens(t)[0], l)[0] for l in R.table_lens(t)[1]}
    assert strides == {'packed NV1', 'packed NV2', 'pool_kernel NV4', 'pool_kernel NV2'}
    hole_bodies = {}
    for (L, D, mode) in R.HOLE_CASES:
        lens = R.cover_lens(R.hole_mask(R.HOLE_N, L, L))
        hole_bodies.setdefault(D, set()).add(R.path_of(True, D, L, lens[0])[1])              # the body of the fully masked row
    assert all(b == set(R.BODIES) for b in hole_bodies.values()) and set(hole_bodies) == {256, 260}


def test_length_tables_pin_both_sides_of_every_boundary():
    L, lens = R.LENGTH_TABLES['ladder']
    assert L == 128 and lens == sorted(lens, reverse=True)
    for lo, hi in ((8, 9), (32, 33), (64, 65)):                      # 8 | 9: single | team, 32 | 33: team | stream, 64 | 65: the second position slot
        assert lo in lens and hi in lens
    assert R.path_of(True, 260, L, 8)[1] != R.path_of(True, 260, L, 9)[1] and R.path_of(True, 260, L, 32)[1] != R.path_of(True, 260, L, 33)[1]
    assert 1 in lens and 128 in lens and 127 in lens
    for name in R.LENGTH_TABLES:                                     # the caller's order is not the sorted one
        Lt, lt = R.table_lens(name)
        assert sorted(lt) == sorted(R.LENGTH_TABLES[name][1]) and max(lt) <= Lt
        if len(lt) > 1:
            assert lt != sorted(lt, reverse=True), name


def test_length_tables_fill_the_last_single_wave_workgroup_every_way():
    counts = {name: R.short_count(True, 260, *R.LENGTH_TABLES[name]) for name in R.LENGTH_TABLES}
    assert {c % 4 for c in counts.values() if c} >= {1, 2, 3}
    assert counts['ladder'] == 6 and counts['ladder-1'] == 5 and counts['ladder-3'] == 3
    assert counts['no_short'] == 0 and counts['one_long'] == 0                                  # tables without a short sequence
    for name in ('short_only', 'short_in_L12', 'one_short'):                                    # ... and with nothing else
        assert counts[name] == len(R.LENGTH_TABLES[name][1])
    assert R.LENGTH_TABLES['short_only'][0] <= R.TEAM_R < R.LENGTH_TABLES['short_in_L12'][0]   # L <= 8: no team is ever used; L = 12: the guard passes
    Lm, mid = R.LENGTH_TABLES['mid']
    assert Lm == 4 * R.TEAM_R and {R.path_of(True, 260, Lm, l)[1] for l in mid} == {'team', 'single'}     # L = 32: off[33] does not exist
    assert R.short_count(False, 260, 128, [1]) is None and R.short_count(True, 516, 128, [1]) is None


def test_packed_cases_are_the_ones_the_suite_is_asked_to_run():
    cases = R.packed_cases()
    assert len(cases) == len(set(cases)) == 18 + 2 + 3 * (len(R.LENGTH_TABLES) - 1)
    for D in (4, 256, 260, 512, 516, 1280):
        for m in R.MODES:
            assert ('ladder', D, m, R.TH_A if m == 'th' else 0, R.TH_A if m == 'th' else 0) in cases
    assert ('ladder', 260, 'th', 4, 12) in cases and ('ladder', 260, 'th', 256, 264) in cases
    assert all(A % 4 == 0 and A <= R.MAX_A and ldth % 4 == 0 and ldth >= A for (_, _, m, A, ldth) in cases if m == 'th')
    assert len(R.dense_cases()) == 2 * 7 * 2 + 2 * 2 + 2
