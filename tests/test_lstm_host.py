"""Host tests of tests/lstm_ref.py, the float64 restatement of the Bi-LSTM recurrence that tests/test_hip_lstm_gpu.py holds the kernels of
csrc/lstm.hip to: against torch.nn.LSTM(bidirectional=True) in float64 on a PackedSequence (h, c_n, and -- through the chain rule from the
hand-written dz -- the gradients of x and of all eight parameters; dz itself through an LSTM whose input projection is the identity), against
the oracle's BiLSTM, and the layout helpers as bijections.

The bar.  torch against itself (ATen's fused CPU LSTM on the PackedSequence against the oracle's explicit time loop, both float64, the shapes
below, h, c_n and every gradient) differs by at most 1.1e-15 of max(1, largest expected magnitude): float64 round-off of sums of up to n * L
terms; the test that measures it requires it to stay below 1e-13.  The restatement is held to RTOL = 1e-12 of the same scale: three orders
over torch's own spread, and many orders below anything a wrong index, gate or sign would produce."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_ref as R

RTOL = 1e-12
NAMES = ['weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0']
NAMES = NAMES + [k + '_reverse' for k in NAMES]
# (n, L, E, H)
SHAPES = [(1, 1, 3, 1), (5, 7, 4, 3), (9, 6, 5, 17), (20, 12, 8, 16), (6, 9, 2, 40)]


def _lens(n, L, g):
    lens = torch.randint(1, L + 1, (n,), generator=g)
    lens[0] = L
    if n > 1:
        lens[1] = 1
    if n > 3:
        lens[3] = lens[2]                                   # a tie
    return lens


def _near(got, exp, what):
    err, scale = float((got - exp).abs().max()), max(1.0, float(exp.abs().max()))
    assert err <= RTOL * scale, '%s: err %.3e (scale %.3e)' % (what, err, scale)
    return err / scale


def _torch_lstm(lstm, x, lens, dH, dc):
    """nn.LSTM on a PackedSequence: (H [n, L, 2h], c_n [n, 2h]) in the caller's row order, and the backward of sum(H dH) + sum(c_n dc)."""
    n, L, _ = x.shape
    out, (_, c_n) = lstm(pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False))
    H, _ = pad_packed_sequence(out, batch_first=True, total_length=L)
    c_n = torch.cat([c_n[0], c_n[1]], dim=1)
    ((H * dH).sum() + (c_n * dc).sum()).backward()
    return H.detach(), c_n.detach()


def _case(shape):
    n, L, E, H = shape
    g = torch.Generator().manual_seed(n * 100 + L)
    lstm = torch.nn.LSTM(E, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for q in lstm.parameters():
            q.copy_(torch.empty(q.shape, dtype=torch.float64).uniform_(-1.5 / H ** 0.5, 1.5 / H ** 0.5, generator=g))
    lens = _lens(n, L, g)
    x = torch.randn(n, L, E, generator=g, dtype=torch.float64)
    mask = (torch.arange(L)[None, :] < lens[:, None])
    dH = torch.randn(n, L, 2 * H, generator=g, dtype=torch.float64) * mask[:, :, None]
    dc = torch.randn(n, 2 * H, generator=g, dtype=torch.float64)
    return lstm, lens, x, mask, dH, dc


def _pre_activations(lstm, x):
    p = {k: getattr(lstm, k).detach() for k in NAMES}
    return torch.stack([x @ p['weight_ih_l0' + s].t() + p['bias_ih_l0' + s] + p['bias_hh_l0' + s] for s in ('', '_reverse')], dim=2)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_restatement_equals_nn_lstm_on_a_packed_sequence(shape):
    n, L, E, H = shape
    lstm, lens, x, mask, dH, dc = _case(shape)
    assert int(lens.min()) == 1 and int(lens.max()) == L
    xr = x.clone().requires_grad_()
    Hexp, cexp = _torch_lstm(lstm, xr, lens, dH, dc)
    w_hh = [lstm.weight_hh_l0.detach(), lstm.weight_hh_l0_reverse.detach()]
    xw = _pre_activations(lstm, x)
    fwd = R.bilstm(xw, w_hh, lens)
    _near(fwd['h'], Hexp, 'h')
    _near(fwd['c_n'], cexp, 'c_n')
    assert float(fwd['h'][~mask].abs().sum()) == 0.0 and float(fwd['gates'][~mask].abs().sum()) == 0.0
    for s in range(n):                                        # c_n is the cell of the last step each direction runs
        assert torch.equal(fwd['c_n'][s, :H], fwd['cell'][s, int(lens[s]) - 1, 0]) and torch.equal(fwd['c_n'][s, H:], fwd['cell'][s, 0, 1])
    # the chain rule from dz to everything autograd differentiates
    dz = R.bilstm_backward(fwd, w_hh, lens, dH, dc)
    assert float(dz[~mask].abs().sum()) == 0.0
    hprev = R.h_before(fwd, lens)
    dx = sum(dz[:, :, d] @ getattr(lstm, 'weight_ih_l0' + s).detach() for d, s in enumerate(('', '_reverse')))
    _near(dx, xr.grad, 'dx')
    for d, s in enumerate(('', '_reverse')):
        _near(torch.einsum('nlp,nle->pe', dz[:, :, d], x), getattr(lstm, 'weight_ih_l0' + s).grad, 'dW_ih' + s)
        _near(torch.einsum('nlp,nlk->pk', dz[:, :, d], hprev[:, :, d]), getattr(lstm, 'weight_hh_l0' + s).grad, 'dW_hh' + s)
        _near(dz[:, :, d].sum(dim=(0, 1)), getattr(lstm, 'bias_ih_l0' + s).grad, 'db_ih' + s)
        _near(dz[:, :, d].sum(dim=(0, 1)), getattr(lstm, 'bias_hh_l0' + s).grad, 'db_hh' + s)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('source', ['both', 'dh_only', 'dcn_only'])
def test_dz_is_the_input_gradient_of_an_identity_projection(shape, source):
    """An nn.LSTM of input width 8H whose W_ih are [I 0] and [0 I] with zero biases takes the pre-activations of both directions as its input:
    its input gradient IS dz, element by element, for each gradient source alone as well."""
    n, L, _, H = shape
    lstm0, lens, _, mask, dH, dc = _case(shape)
    g = torch.Generator().manual_seed(7)
    xw = torch.randn(n, L, 2, 4 * H, generator=g, dtype=torch.float64)
    if source == 'dh_only':
        dc = torch.zeros_like(dc)
    if source == 'dcn_only':
        dH = torch.zeros_like(dH)
    lstm = torch.nn.LSTM(8 * H, H, batch_first=True, bidirectional=True).double()
    eye = torch.eye(4 * H, dtype=torch.float64)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([eye, torch.zeros_like(eye)], dim=1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat([torch.zeros_like(eye), eye], dim=1))
        for k in NAMES:
            if 'bias' in k:
                getattr(lstm, k).zero_()
            if 'weight_hh' in k:
                getattr(lstm, k).copy_(getattr(lstm0, k))
    xin = xw.reshape(n, L, 8 * H).clone().requires_grad_()
    Hexp, cexp = _torch_lstm(lstm, xin, lens, dH, dc)
    w_hh = [lstm.weight_hh_l0.detach(), lstm.weight_hh_l0_reverse.detach()]
    fwd = R.bilstm(xw, w_hh, lens)
    _near(fwd['h'], Hexp, 'h')
    _near(fwd['c_n'], cexp, 'c_n')
    dz = R.bilstm_backward(fwd, w_hh, lens, None if source == 'dcn_only' else dH, None if source == 'dh_only' else dc)
    _near(dz.reshape(n, L, 8 * H), xin.grad, 'dz')
    assert float(dz.abs().max()) > 1e-3


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_restatement_equals_the_oracles_bilstm_and_torch_equals_itself(shape):
    from oracle.nnr_oracle import BiLSTM
    n, L, E, H = shape
    lstm, lens, x, mask, dH, dc = _case(shape)
    ref = BiLSTM(E, H).double()
    ref.load_state_dict(lstm.state_dict())
    xo = x.clone().requires_grad_()
    Ho, co = ref(xo, lens)
    ((Ho * dH).sum() + (co * dc).sum()).backward()
    w_hh = [lstm.weight_hh_l0.detach(), lstm.weight_hh_l0_reverse.detach()]
    fwd = R.bilstm(_pre_activations(lstm, x), w_hh, lens)
    _near(fwd['h'], Ho.detach(), 'h')
    _near(fwd['c_n'], co.detach(), 'c_n')
    dz = R.bilstm_backward(fwd, w_hh, lens, dH, dc)
    dx = sum(dz[:, :, d] @ getattr(lstm, 'weight_ih_l0' + s).detach() for d, s in enumerate(('', '_reverse')))
    _near(dx, xo.grad, 'dx')
    # torch against itself: what the bar is stated from (module docstring)
    xt = x.clone().requires_grad_()
    Ht, ct = _torch_lstm(lstm, xt, lens, dH, dc)
    worst = max(_near(Ht, Ho.detach(), 'torch h'), _near(ct, co.detach(), 'torch c_n'), _near(xt.grad, xo.grad, 'torch dx'))
    worst = max([worst] + [_near(getattr(lstm, k).grad, getattr(ref, k).grad, 'torch d' + k) for k in NAMES])
    print('torch against itself at %s: %.2e of scale' % (shape, worst))
    assert worst <= RTOL / 10                                 # the bar leaves an order of magnitude over torch's own spread


@pytest.mark.parametrize('H', [1, 15, 16, 17, 200, 256])
def test_p_order_is_a_bijection_onto_the_unpadded_columns(H):
    HP, NP = R.padded(H)
    assert HP % 16 == 0 and HP - 16 < H <= HP and NP == 4 * HP
    cols = R.gate_columns(H)
    assert cols.shape == (4 * H,) and len(set(cols.tolist())) == 4 * H and int(cols.min()) >= 0 and int(cols.max()) < NP
    # the columns left over are exactly those of the padded units H .. HP - 1, and a unit's four gates are adjacent
    rest = sorted(set(range(NP)) - set(cols.tolist()))
    assert rest == sorted(R.p_index(u, g) for u in range(H, HP) for g in range(4))
    for u in (0, H // 2, H - 1):
        assert [R.p_index(u, g) for g in range(4)] == list(range(R.p_index(u, 0), R.p_index(u, 0) + 4)) and R.p_index(u, 0) % 4 == 0
    assert int(cols[2 * H + (H - 1)]) == R.p_index(H - 1, 2)


@pytest.mark.parametrize('n,L', [(1, 1), (5, 7), (37, 12), (16, 3)])
def test_packed_rows_are_a_bijection_onto_the_valid_tokens(n, L):
    g = torch.Generator().manual_seed(n + L)
    lens = _lens(n, L, g)
    order, rank = R.length_order(lens)
    bs, off = R.batch_sizes(lens, L)
    assert torch.equal(rank[order], torch.arange(n)) and bool((lens[order][:-1] >= lens[order][1:]).all())
    packed = pack_padded_sequence(torch.zeros(n, L, 1), lens, batch_first=True, enforce_sorted=False)
    assert torch.equal(packed.batch_sizes, bs[:int(lens.max())]) and int(off[L]) == int(lens.sum())
    rows = [int(R.packed_row(off, rank, s, t)) for s in range(n) for t in range(int(lens[s]))]
    assert sorted(rows) == list(range(int(lens.sum())))
    for s in range(n):
        for t in range(int(lens[s])):
            assert int(off[t]) <= int(R.packed_row(off, rank, s, t)) < int(off[t + 1])
    # equal lengths keep their original order (the planner's sort is stable)
    for a in range(n):
        for b in range(a + 1, n):
            if lens[a] == lens[b]:
                assert rank[a] < rank[b]


def test_plain_float32_leaves_three_quarters_of_every_bar():
    """The GPU file's bars (2e-5 forward, 1e-4 for dz) against what float32 itself costs: the restatement run in plain float32 on the host, at
    the longest problems of each kernel family, uses less than a quarter of a bar (in fact about 1 %: tests/test_hip_lstm_gpu.py's docstring)."""
    import test_hip_lstm_gpu as G
    assert set(G.LARGEST) <= set(G.all_specs())
    for spec in G.LARGEST:
        p = G.problem(spec)
        f32 = R.bilstm(p['xw'], p['w_hh'], p['lens'], dtype=torch.float32)
        dz32 = R.bilstm_backward(f32, p['w_hh'], p['lens'], p['dh'], p['dcn'])
        assert f32['h'].dtype == torch.float32 and dz32.dtype == torch.float32
        for k in ('h', 'c_n', 'gates', 'cell'):
            e = p['fwd'][k]
            assert float((f32[k].double() - e).abs().max()) <= 0.25 * G.FWD_TOL * max(1.0, float(e.abs().max())), (spec[:3], k)
        e = G.expected_dz(spec)
        assert float((dz32.double() - e).abs().max()) <= 0.25 * G.DZ_TOL * max(1.0, float(e.abs().max())), (spec[:3], 'dz')
