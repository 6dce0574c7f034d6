"""The Bi-LSTM recurrence kernels (csrc/lstm.hip behind nnr_lstm_fwd / nnr_lstm_bwd) against the float64 restatement tests/lstm_ref.py
(pinned to torch.nn.LSTM on a PackedSequence by tests/test_lstm_host.py), fed DIRECTLY: the gates buffer is filled with the reference's
pre-activations in p-order and packed rows, there is no input GEMM and no weight-gradient GEMM between a kernel and the comparison.  Every
case compares hout, c_n, the activated gates, the cell states and -- after the backward -- dz (the gates buffer again), and asserts: no exchange
time-out, everything finite (padded units and columns included), and rows at and past the plan's token count, pre-filled with a marker,
untouched bit for bit in hout, cell and gates after either pass.

Families: the one-CU kernels launch_rec<UB> for UB = 1 .. 16 (4 waves up to H = 64, 16 waves from H = 65), and the CU-pair kernels (16-row
bodies, 4-row quad bodies, the one-token shortcut; forward and backward) that nnr_lstm_fwd / _bwd take for every even H in 194 .. 208 when every
problem carries a `sync` workspace.  nnr_amd.ops hands out workspaces at H = 200 only, so at H = 194 and 208 the test supplies its own.

Bars: the `close` of tests/test_hip_ops_gpu.py, 2e-5 of max(1, largest expected magnitude) for the forward quantities and 1e-4 for dz, at
xw ~ N(0, 1), w_hh uniform in +-1.5 / sqrt(H), dh, dc_n ~ N(0, 1).  The room they leave: the restatement's own arithmetic in plain float32
torch on the CPU (lstm_ref.bilstm(..., dtype=torch.float32)), over every problem of all_specs(), differs from float64 by at most, in units
of max(1, largest expected magnitude): h 1.9e-7 (H = 200, saturated), c_n 1.6e-7 (H = 65, L = 24), activated gates 1.6e-7 (H = 256), cell
1.8e-7 (H = 194, n = 70, L = 24), dz 2.3e-7 (H = 208, L = 70) -- 1 % of the forward bar and 0.3 % of the gradient bar, far below the
quarter at which a shape would have to shrink.  tests/test_lstm_host.py::test_plain_float32_leaves_three_quarters_of_every_bar re-measures
the longest problems of each family on the host."""
import functools

import pytest
import torch

import lstm_ref as R
from test_hip_ops_gpu import close, _lengths

pytestmark = pytest.mark.gpu

FWD_TOL, DZ_TOL = 2e-5, 1e-4
MARK = 12345.678                     # rows past the plan's token count are pre-filled with this and must come back bit for bit
GUARD = 3                            # such rows exist even when every sequence is full
SAT = (100.0, -100.0, 1e30, -1e30)

ONE_CU_H = [1, 15, 16, 17, 48, 64, 65, 112, 199, 200, 209, 250, 256]
EDGE_H = [17, 64, 65, 256]                                   # both sides of the 4 / 16 wave switch, padded units, the limit
EDGE_SHAPES = [(1, 1, 'ragged'), (1, 7, 'ragged'), (16, 5, 'ragged'), (17, 5, 'ragged'), (17, 5, 'equal'), (17, 5, 'ones')]
PAIR_H = [194, 200, 208]                                     # the two ends of the pair kernels' interval and the product's size
PAIR_SHAPES = [(1, 2, 'ragged'), (4, 9, 'ragged'), (5, 9, 'ragged'), (16, 6, 'ragged'), (17, 7, 'ragged'), (40, 24, 'ragged'),
               (33, 5, 'ones'), (20, 8, 'equal'), (16, 11, 'long_row'), (40, 9, 'ones_tail')]
# 12 sequences of which 5 / 9 are longer than T = 3: the last quad tile is short and holds sequences no longer than T
BS5 = (3, 8, 1, 7, 3, 6, 2, 5, 2, 4, 1, 3)
BS9 = (8, 2, 8, 7, 3, 6, 6, 5, 1, 5, 4, 4)
LONG70 = (65, 70, 1, 69, 33, 66)
MULTI = [(20, 8), (70, 24), (5, 3), (33, 1)]
SPLIT_H = [65, 200, 194]                                     # separated gradient sources, saturation: one-CU (16 waves) and pair


# the problems with the most steps / widest sums of each family: where plain float32 strays furthest
LARGEST = [(256, 37, 12, 'ragged'), (208, 40, 24, 'ragged'), (208, 6, 70, LONG70), (194, 70, 24, 'ragged'), (200, 20, 24, 'reversed'), (200, 20, 10, 'sat')]


def all_specs():
    """Every (H, n, L, kind) this file runs."""
    out = [(H, 37, 12, 'ragged') for H in ONE_CU_H]
    out += [(H, n, L, kind) for H in EDGE_H for n, L, kind in EDGE_SHAPES]
    out += [(H, n, L, kind) for H in PAIR_H for n, L, kind in PAIR_SHAPES]
    out += [(H, 12, 8, lens) for H in PAIR_H for lens in (BS5, BS9)]
    out += [(208, 6, 70, LONG70)]
    out += [(H, n, L, 'ragged') for H in (48, 200, 194) for n, L in MULTI]
    out += [(H, 20, 24, 'reversed') for H in SPLIT_H] + [(H, 20, 10, 'sat') for H in SPLIT_H]
    return list(dict.fromkeys(out))


def lengths_of(n, L, kind):
    if isinstance(kind, tuple):
        return torch.tensor(kind)
    if kind == 'equal':
        return torch.full((n,), L)
    if kind == 'ones':
        return torch.ones(n, dtype=torch.long)
    if kind == 'long_row':                                   # one 16-row tile: one long row, fifteen rows of one token
        lens = torch.ones(n, dtype=torch.long)
        lens[5] = L
        return lens
    if kind == 'reversed':                                   # ascending: the sorted order differs from the original one at every position
        return torch.arange(n) + (L - n + 1)
    lens = _lengths(n, L, n + L) if n > 1 else torch.tensor([L])          # forced: lens[0] = L, lens[1] = 1
    if kind == 'ones_tail':                                  # the tiles behind the first are whole tiles of one-token sequences
        lens[10:] = 1
    return lens


@functools.lru_cache(maxsize=None)
def problem(spec):
    """fp32 inputs of one (H, n, L, kind) and the float64 results for each gradient source (computed once, shared, never modified)."""
    H, n, L, kind = spec
    lens = lengths_of(n, L, kind)
    assert lens.shape == (n,) and int(lens.min()) >= 1 and int(lens.max()) <= L
    g = torch.Generator().manual_seed(H * 7919 + n * 131 + L)
    xw = torch.randn(n, L, 2, 4 * H, generator=g)
    k = 1.5 / H ** 0.5
    w_hh = torch.empty(2, 4 * H, H).uniform_(-k, k, generator=g)
    dh = torch.randn(n, L, 2 * H, generator=g)
    dcn = torch.randn(n, 2 * H, generator=g)
    sat_cols = None
    if kind == 'sat':
        # unit u with u % 32 = 4 k + gate (k < 4) has that gate's column at SAT[k], in every row and both directions; units with u % 32 >= 16
        # stay normal
        unit = torch.arange(H)
        sat_cols = torch.zeros(4 * H, dtype=torch.bool)
        for kk, val in enumerate(SAT):
            for gate in range(4):
                u = unit[unit % 32 == 4 * kk + gate]
                xw[:, :, :, gate * H + u] = val
                sat_cols[gate * H + u] = True
    mask = torch.arange(L)[None, :] < lens[:, None]
    fwd = R.bilstm(xw, w_hh, lens)
    return dict(spec=spec, H=H, n=n, L=L, lens=lens, mask=mask, xw=xw, w_hh=w_hh, dh=dh, dcn=dcn, fwd=fwd, sat_cols=sat_cols)


@functools.lru_cache(maxsize=None)
def expected_dz(spec, grads='both'):
    p = problem(spec)
    return R.bilstm_backward(p['fwd'], p['w_hh'], p['lens'], None if grads == 'dcn' else p['dh'], None if grads.startswith('dh') else p['dcn'])


# ---------------------------------------------------------------------------------------------- driving the kernels
@functools.lru_cache(maxsize=None)
def _weights(spec):
    from nnr_amd import ops
    p = problem(spec)
    H = p['H']
    zeros = [torch.zeros(4 * H, 1), None, torch.zeros(4 * H), torch.zeros(4 * H)]          # E = 1: the input projection is not part of this file
    params = [t.cuda() for d in (0, 1) for t in (zeros[0], p['w_hh'][d].contiguous(), zeros[2], zeros[3])]
    return ops.LstmPacked(params, H, 1)


def _set_env(monkeypatch, quad_T=None, dbg=None):
    for k, v in (('NNR_LSTM_QUAD_T', quad_T), ('NNR_LSTM_DBG', dbg), ('NNR_LSTM_PAIR', None)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _item(spec, own_ws):
    """Buffers of one problem as nnr_lstm_fwd takes them, from the restatement's inputs."""
    from nnr_amd import ops, _lib
    p = problem(spec)
    H, n, L, lens, mask = p['H'], p['n'], p['L'], p['lens'], p['mask']
    HP, NP = R.padded(H)
    plan = ops.SeqPlan(mask.clone().cuda(), None)
    order, rank = R.length_order(lens)
    bs, off = R.batch_sizes(lens, L)
    # the helpers state the header's contract; the planner (tests of its own) must say the same
    assert torch.equal(plan.off.cpu().long(), off) and torch.equal(plan.rank.cpu().long(), rank) and torch.equal(plan.order.cpu().long(), order)
    total = int(off[L])
    rows = torch.stack([R.packed_row(off, rank, torch.arange(n), t) for t in range(L)], dim=1)       # [n, L], meaningful where mask
    nrows = n * L + GUARD
    cols = R.gate_columns(H)
    gates = torch.full((nrows, 2 * NP), MARK)
    gates[:total] = 0.0                                                                          # padded columns are zero
    for d in (0, 1):
        blk = torch.zeros(total, NP)
        blk[rows[mask][:, None], cols[None, :]] = p['xw'][mask][:, d]
        gates[:total, d * NP:(d + 1) * NP] = blk
    nan = float('nan')
    cell = torch.full((nrows, 2 * HP), MARK)
    cell[:total] = nan                                                                           # every valid element must be written
    hout = torch.full((nrows, 2 * H), MARK)
    hout[:total] = nan
    it = dict(plan=plan, w=_weights(spec), gates=gates.cuda(), cell=cell.cuda(), hout=hout.cuda(), cn=torch.full((n, 2 * H), nan).cuda(),
              name='lstm_gpu_test')
    if own_ws:
        it['sync'] = torch.zeros(_lib.lib().nnr_lstm_sync_bytes(n) // 4, dtype=torch.int32, device='cuda')
    aux = dict(p=p, total=total, rows=rows, order=order, rank=rank, cols=cols, own_ws=it.get('sync'))
    return it, aux


def _exchange_timeouts(items):
    """Time-outs the last launch recorded in the diagnostics block of each item's workspace (0 without one)."""
    from nnr_amd import _lib
    return sum(int(it['sync'][_lib.lib().nnr_lstm_sync_diag_offset(it['plan'].n) // 4]) for it in items if it.get('sync') is not None)


def run(specs, own_ws=False, grads='both'):
    """Forward and backward launch of the problems `specs` (one launch each); returns per problem the raw buffers on the host."""
    from nnr_amd import ops
    H = specs[0][0]
    ops._timeout_counter(torch.device('cuda', torch.cuda.current_device()))
    ops.lstm_sync_timeouts(reset=True)
    built = [_item(s, own_ws) for s in specs]
    items = [it for it, _ in built]
    ops.lstm_fwd(items, H)
    torch.cuda.synchronize()
    assert ops.lstm_sync_timeouts() == 0 and _exchange_timeouts(items) == 0, 'exchange time-out in the forward launch'
    outs = []
    for it, aux in built:
        outs.append(dict(aux, item=it, hout=it['hout'].cpu(), cn=it['cn'].cpu(), act=it['gates'].cpu(), cell=it['cell'].cpu()))
        p, total = aux['p'], aux['total']
        dh = torch.zeros(p['n'] * p['L'] + GUARD, 2 * p['H'])
        if grads != 'dcn':
            dh[aux['rows'][p['mask']]] = p['dh'][p['mask']]
        it['dh'] = dh.cuda()
        if grads == 'both' or grads == 'dcn':
            it['dcn'] = p['dcn'][aux['order']].contiguous().cuda()                 # sorted order
        elif grads == 'dh':
            it['dcn'] = torch.zeros(p['n'], 2 * p['H']).cuda()
        else:
            assert grads == 'dh_null' and 'dcn' not in it
    ops.lstm_bwd(items, H)
    torch.cuda.synchronize()
    assert ops.lstm_sync_timeouts() == 0 and _exchange_timeouts(items) == 0, 'exchange time-out in the backward launch'
    for o in outs:
        o['dz'] = o['item']['gates'].cpu()
        o['hout_after'], o['cell_after'] = o['item']['hout'].cpu(), o['item']['cell'].cpu()
    return outs


def check(o, tag, grads='both'):
    """One problem's buffers against the restatement, and everything every case asserts."""
    p, total, rows, rank, cols = o['p'], o['total'], o['rows'], o['rank'], o['cols']
    H, mask, fwd = p['H'], p['mask'], p['fwd']
    HP, NP = R.padded(H)
    idx = rows[mask]
    for k in ('hout', 'cn', 'act', 'cell', 'dz'):
        live = o[k] if k == 'cn' else o[k][:total]
        assert bool(torch.isfinite(live).all()), '%s: %s is not finite (padded units / columns included)' % (tag, k)
    marker = _bits(torch.full((1,), MARK))
    for k in ('hout', 'act', 'cell', 'dz', 'hout_after', 'cell_after'):
        assert bool((_bits(o[k][total:]) == marker).all()), '%s: rows past the token count of %s were written' % (tag, k)
    assert torch.equal(_bits(o['hout_after']), _bits(o['hout'])) and torch.equal(_bits(o['cell_after']), _bits(o['cell'])), tag + ': backward wrote h / cell'
    dz = expected_dz(p['spec'], grads)
    got = torch.stack([o['dz'][idx][:, d * NP + cols] for d in (0, 1)], dim=1)
    pairs = [('hout', o['hout'][idx], fwd['h'][mask], FWD_TOL), ('c_n', o['cn'][rank], fwd['c_n'], FWD_TOL)]
    for d in (0, 1):
        pairs.append(('activated gates, direction %d' % d, o['act'][idx][:, d * NP + cols], fwd['gates'][mask][:, d], FWD_TOL))
        pairs.append(('cell, direction %d' % d, o['cell'][idx][:, d * HP:d * HP + H], fwd['cell'][mask][:, d], FWD_TOL))
    pairs.append(('dz', got, dz[mask], DZ_TOL))
    print(tag + ': ' + '; '.join('%s %.1e of %.1e' % (k.replace(', direction ', ' d'), float((a.double() - e).abs().max()),
                                                      tol * max(1.0, float(e.abs().max()))) for k, a, e, tol in pairs))
    for k, a, e, tol in pairs:
        close(a, e, tol=tol, what=tag + ' ' + k)
    return got


def same_bits(a, b, tag):
    for k in ('hout', 'cn', 'act', 'cell', 'dz'):
        assert torch.equal(_bits(a[k]), _bits(b[k])), '%s: %s differs in bits' % (tag, k)


def quad_settings(L):
    return list(dict.fromkeys(['0', '3', str(L - 1), str(L), None]))


def _pair_was_taken(o):
    """The pair kernels leave their placement handshake in a workspace the test zero-filled (any tile longer than one step)."""
    return o['own_ws'] is not None and bool(o['own_ws'].any())


# ---------------------------------------------------------------------------------------------- 1. the one-CU family
@pytest.mark.parametrize('H', ONE_CU_H)
def test_one_cu_kernels_at_every_block_count(H, monkeypatch):
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', False)
    _set_env(monkeypatch)
    (o,) = run([(H, 37, 12, 'ragged')])
    assert 'sync' not in o['item']
    check(o, 'one-CU H=%d' % H)


@pytest.mark.parametrize('H', EDGE_H)
def test_one_cu_kernels_at_the_tile_edges(H, monkeypatch):
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', False)
    _set_env(monkeypatch)
    for n, L, kind in EDGE_SHAPES:
        (o,) = run([(H, n, L, kind)])
        check(o, 'one-CU H=%d %s' % (H, (n, L, kind)))


def test_odd_hidden_size_never_pairs(monkeypatch):
    """H = 199 has 13 unit blocks like H = 200, but the pair kernels take even sizes only: with a workspace it still runs the one-CU kernel."""
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', True)
    _set_env(monkeypatch)
    spec = (199, 37, 12, 'ragged')
    (o,) = run([spec], own_ws=True)
    check(o, 'H=199 with a workspace')
    assert o['item']['sync'] is o['own_ws'] and not _pair_was_taken(o)
    monkeypatch.setattr(ops, 'LSTM_PAIR', False)
    (alone,) = run([spec])
    same_bits(o, alone, 'H=199 with and without a workspace')


def test_unsupported_sizes_and_problem_counts_are_refused(monkeypatch):
    from nnr_amd import ops, _lib
    monkeypatch.setattr(ops, 'LSTM_PAIR', False)
    _set_env(monkeypatch)
    for H in (0, 257, -16):
        with pytest.raises(_lib.NnrHipError):
            ops.lstm_dims(H)
        with pytest.raises(_lib.NnrHipError):
            ops.LstmPacked([torch.zeros(4, device='cuda')] * 8, H, 1)
    assert ops.lstm_dims(256) == (16, 256, 1024) and ops.lstm_dims(1) == (1, 16, 64) and ops.lstm_dims(194) == (13, 208, 832)
    it, aux = _item((256, 1, 7, 'ragged'), False)
    it['dh'] = torch.zeros_like(it['hout'])
    before = {k: it[k].clone() for k in ('gates', 'cell', 'hout', 'cn')}
    for fn in (ops.lstm_fwd, ops.lstm_bwd):
        for H in (257, 0):
            with pytest.raises(_lib.NnrHipError, match='code %d' % _lib.NNR_ERR_UNSUPPORTED):
                fn([it], H)
        for items in ([], [it] * 5):
            with pytest.raises(_lib.NnrHipError, match='code %d' % _lib.NNR_ERR_ARG):
                fn(items, 256)
    torch.cuda.synchronize()
    for k, v in before.items():                               # nothing was launched
        assert torch.equal(_bits(it[k]), _bits(v)), k


# ---------------------------------------------------------------------------------------------- 2. the pair family
@pytest.mark.parametrize('shape', PAIR_SHAPES, ids=lambda s: '%dx%d_%s' % s)
@pytest.mark.parametrize('H', PAIR_H)
def test_pair_kernels_at_the_tile_edges_and_quad_thresholds(H, shape, monkeypatch):
    """16-row bodies, quad bodies and the one-token shortcut, forward and backward, at NNR_LSTM_QUAD_T = 0, 3, L - 1, L and unset; odd and even L
    (both step parities of the exchange slots)."""
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', True)
    n, L, kind = shape
    spec = (H, n, L, kind)
    for quad_T in quad_settings(L):
        _set_env(monkeypatch, quad_T=quad_T)
        (o,) = run([spec], own_ws=True)
        tag = 'pair H=%d %s quad_T=%s' % (H, shape, quad_T)
        check(o, tag)
        if H == 200:
            assert o['item']['sync'] is not o['own_ws'], tag       # ops hands out its own workspace at the product's size
        elif int(problem(spec)['lens'].max()) > 1:
            assert _pair_was_taken(o), tag + ': the entry did not take the pair kernels'


@pytest.mark.parametrize('H', PAIR_H)
def test_pair_kernels_on_the_cross_xcd_exchange(H, monkeypatch):
    """NNR_LSTM_DBG=64: the fabric flavour of the exchange, which a pair takes when its halves land on different XCDs."""
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', True)
    for quad_T in ('0', '3'):
        _set_env(monkeypatch, quad_T=quad_T, dbg=64)
        (o,) = run([(H, 40, 24, 'ragged')], own_ws=True)
        check(o, 'pair fabric H=%d quad_T=%s' % (H, quad_T))
        _set_env(monkeypatch, quad_T=quad_T)
        (same,) = run([(H, 40, 24, 'ragged')], own_ws=True)
        same_bits(o, same, 'fabric against same-XCD exchange, H=%d' % H)


@pytest.mark.parametrize('lens', [BS5, BS9], ids=['bs5', 'bs9'])
@pytest.mark.parametrize('H', PAIR_H)
def test_pair_kernels_with_a_short_last_quad(H, lens, monkeypatch):
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', True)
    _set_env(monkeypatch, quad_T='3')
    spec = (H, 12, 8, lens)
    bs, _ = R.batch_sizes(problem(spec)['lens'], 8)
    assert int(bs[3]) == (5 if lens is BS5 else 9)
    (o,) = run([spec], own_ws=True)
    check(o, 'pair H=%d bs[T]=%d' % (H, int(bs[3])))


def test_pair_kernels_past_64_steps(monkeypatch):
    from nnr_amd import ops
    monkeypatch.setattr(ops, 'LSTM_PAIR', True)
    for quad_T in (None, '0'):
        _set_env(monkeypatch, quad_T=quad_T)
        (o,) = run([(208, 6, 70, LONG70)], own_ws=True)
        check(o, 'pair H=208 L=70 quad_T=%s' % quad_T)
        assert _pair_was_taken(o)


# ---------------------------------------------------------------------------------------------- 3. several problems per launch
@pytest.mark.parametrize('H', [48, 200, 194])
def test_problems_of_one_launch_equal_the_same_problems_alone(H, monkeypatch):
    """(problem, direction) interleave of the pair grid, surplus tiles of the smaller problems, first and last problem: every problem's
    buffers equal, bit for bit, its launch alone at the same NNR_LSTM_QUAD_T; and once without the variable, where the largest n of the launch
    selects the threshold, to the float64 bars."""
    from nnr_amd import ops
    pair = H != 48
    monkeypatch.setattr(ops, 'LSTM_PAIR', pair)
    _set_env(monkeypatch, quad_T='3')
    specs = [(H, n, L, 'ragged') for n, L in MULTI]
    alone = [run([s], own_ws=pair)[0] for s in specs]
    for s, o in zip(specs, alone):
        check(o, 'alone %s' % (s,))
    for nprob in (2, 3, 4):
        for rot in (0, 1):                                      # every problem is the first and the last of some launch
            sel = [(i + rot) % nprob for i in range(nprob)]
            outs = run([specs[i] for i in sel], own_ws=pair)
            for i, o in zip(sel, outs):
                tag = 'H=%d problem %s in a launch of %d (rotation %d)' % (H, specs[i][1:3], nprob, rot)
                check(o, tag)
                same_bits(o, alone[i], tag)
                assert not pair or H == 200 or specs[i][2] == 1 or _pair_was_taken(o), tag
    _set_env(monkeypatch)
    for o, s in zip(run(specs, own_ws=pair), specs):
        check(o, 'H=%d problem %s of 4, threshold from the largest n' % (H, s[1:3]))


# ---------------------------------------------------------------------------------------------- 4. separated gradient sources
@pytest.mark.parametrize('H,grads', [(H, g) for H in SPLIT_H for g in ('dh', 'dcn')] + [(65, 'dh_null')])
def test_each_gradient_source_alone(H, grads, monkeypatch):
    """dh with dc_n zero (or absent: a null pointer), and dc_n with dh zero, on a batch whose sorted order differs from the original order at
    every position: dc_n is indexed in sorted order, dh in packed rows."""
    from nnr_amd import ops
    pair = H != 65
    monkeypatch.setattr(ops, 'LSTM_PAIR', pair)
    spec = (H, 20, 24, 'reversed')
    order, _ = R.length_order(problem(spec)['lens'])
    assert bool((order != torch.arange(20)).all())
    for quad_T in (('0', None) if pair else (None,)):
        _set_env(monkeypatch, quad_T=quad_T)
        (o,) = run([spec], own_ws=pair, grads=grads)
        got = check(o, 'H=%d %s only, quad_T=%s' % (H, grads, quad_T), grads=grads)
        assert float(got.abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- 5. saturation
@pytest.mark.parametrize('H', SPLIT_H)
def test_saturated_gates_stay_finite_and_exact(H, monkeypatch):
    """Gate columns at +-100 and +-1e30 (exp2 overflows, rcp of infinity): outputs within the forward bar, dz of those columns within the
    gradient bar of the float64 result -- which is zero."""
    from nnr_amd import ops
    pair = H != 65
    monkeypatch.setattr(ops, 'LSTM_PAIR', pair)
    spec = (H, 20, 10, 'sat')
    p = problem(spec)
    sat = p['sat_cols']
    assert float(expected_dz(spec)[p['mask']][:, :, sat].abs().max()) <= 1e-30 and int(sat.sum()) >= 16
    for quad_T in (('0', '3') if pair else (None,)):
        _set_env(monkeypatch, quad_T=quad_T)
        (o,) = run([spec], own_ws=pair)
        got = check(o, 'saturated H=%d quad_T=%s' % (H, quad_T))
        scale = max(1.0, float(expected_dz(spec).abs().max()))
        assert float(got[:, :, sat].abs().max()) <= DZ_TOL * scale
        assert float(got[:, :, ~sat].abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- 6. pack and unpack
@pytest.mark.parametrize('E', [1, 12])
@pytest.mark.parametrize('H', [1, 17, 64, 200, 208, 250])
def test_pack_and_unpack_are_the_stated_permutation(H, E):
    """w_ihp / b_p: p-order rows, b_ih + b_hh, zeros in the rows of padded units; w_ihp_t its exact transpose.  nnr_lstm_unpack_grads: the
    reference layout exactly (padded rows, filled with non-zero values, ignored), overwrite and accumulate, and zero_src."""
    from nnr_amd import ops, _lib
    g = torch.Generator().manual_seed(H * 13 + E)
    shapes = [(4 * H, E), (4 * H, H), (4 * H,), (4 * H,)] * 2
    params = [torch.randn(s, generator=g) for s in shapes]
    w = ops.LstmPacked([t.cuda() for t in params], H, E)
    HP, NP = R.padded(H)
    cols = R.gate_columns(H)
    assert (w.HP, w.NP) == (HP, NP)
    w_ihp, b_p = torch.zeros(2 * NP, E), torch.zeros(2 * NP)
    for d in (0, 1):
        w_ihp[d * NP + cols] = params[4 * d]
        b_p[d * NP + cols] = params[4 * d + 2] + params[4 * d + 3]
    assert torch.equal(w.w_ihp.cpu(), w_ihp) and torch.equal(w.b_p.cpu(), b_p) and torch.equal(w.w_ihp_t.cpu(), w_ihp.t().contiguous())
    # unpack
    packed = [torch.randn(2 * NP, E, generator=g) + 3.0, torch.randn(2 * NP, generator=g) + 3.0, torch.randn(2, NP, H, generator=g) + 3.0]
    assert all(bool((t != 0).all()) for t in packed)
    exp = []
    for d in (0, 1):
        exp += [packed[0][d * NP + cols], packed[2][d][cols], packed[1][d * NP + cols], packed[1][d * NP + cols]]
    dev = [t.cuda() for t in packed]
    grads = [torch.full(s, 7.0, device='cuda') for s in shapes]
    _lib.check(_lib.lib().nnr_lstm_unpack_grads(*[ops._p(t) for t in dev], H, E, *[ops._p(t) for t in grads], 0, 0, ops._s()), 'unpack (overwrite)')
    for got, e in zip(grads, exp):
        assert torch.equal(got.cpu(), e)
    grads = [torch.zeros(s, device='cuda') for s in shapes]
    ops.lstm_unpack_grads(*dev, H, E, grads)
    for got, e in zip(grads, exp):
        assert torch.equal(got.cpu(), e)
    ops.lstm_unpack_grads(*dev, H, E, grads)                  # accumulates
    for got, e in zip(grads, exp):
        assert torch.equal(got.cpu(), e + e)
    for t, src in zip(dev, packed):
        assert torch.equal(t.cpu(), src)                      # the packed buffers are left alone without zero_src
    ops.lstm_unpack_grads(*dev, H, E, grads, zero_src=True)
    for got, e in zip(grads, exp):
        assert torch.equal(got.cpu(), (e + e) + e)
    for t in dev:
        assert float(t.abs().max()) == 0.0                    # padded rows included
