"""Float64 restatement of the Bi-LSTM RECURRENCE alone (nn.LSTM(bidirectional=True) on a PackedSequence, newsEncoders.py:119-127, without
its input projection): what nnr_lstm_fwd / nnr_lstm_bwd (csrc/lstm.hip) compute between the input GEMM and the weight-gradient GEMMs.  Plain
loops over sequences and steps, the backward written out by hand (no autograd).  tests/test_lstm_host.py pins it to torch.nn.LSTM and to the
oracle's BiLSTM; tests/test_hip_lstm_gpu.py compares the kernels with it.  The index helpers at the end state the kernels' layouts from the
contract of include/nnr_hip.h; nothing here is read from the library."""
import torch


def f64(t):
    return (t if torch.is_tensor(t) else torch.as_tensor(t)).detach().cpu().double()


def _sig(x):
    return torch.sigmoid(x)


def _steps(length, reverse):
    return range(length - 1, -1, -1) if reverse else range(length)


def bilstm(xw, w_hh, lens, dtype=torch.float64):
    """xw [n, L, 2, 4H]: pre-activations x.W_ih^T + b_ih + b_hh of both directions in nn.LSTM's gate order (i, f, g, o); w_hh: the two
    [4H, H] recurrent matrices (forward, reverse); lens [n] >= 1.  Returns
      h [n, L, 2H] (forward | reverse, zero past the length),  c_n [n, 2H] (the cell after the last step each direction runs),
      gates [n, L, 2, 4H] (activated: s(i), s(f), tanh(g), s(o)),  cell [n, L, 2, H] (c_t).
    dtype=torch.float32 runs the same arithmetic in plain float32: the room a float32 kernel needs under a bar."""
    xw = f64(xw).to(dtype)
    w = [f64(w_hh[0]).to(dtype), f64(w_hh[1]).to(dtype)]
    n, L, _, H4 = xw.shape
    H = H4 // 4
    h_out = xw.new_zeros(n, L, 2 * H)
    c_n = xw.new_zeros(n, 2 * H)
    gates = torch.zeros_like(xw)
    cell = xw.new_zeros(n, L, 2, H)
    for s in range(n):
        for d in (0, 1):
            h = xw.new_zeros(H)
            c = xw.new_zeros(H)
            for t in _steps(int(lens[s]), d == 1):
                z = xw[s, t, d] + w[d] @ h
                i, f, g, o = _sig(z[:H]), _sig(z[H:2 * H]), torch.tanh(z[2 * H:3 * H]), _sig(z[3 * H:])
                c = f * c + i * g
                h = o * torch.tanh(c)
                gates[s, t, d] = torch.cat([i, f, g, o])
                cell[s, t, d] = c
                h_out[s, t, d * H:(d + 1) * H] = h
            c_n[s, d * H:(d + 1) * H] = c
    return dict(h=h_out, c_n=c_n, gates=gates, cell=cell)


def bilstm_backward(fwd, w_hh, lens, dh=None, dc_n=None):
    """dz [n, L, 2, 4H]: the gradient with respect to the pre-activations xw, for upstream dh [n, L, 2H] (entries past the length are
    ignored) and dc_n [n, 2H]; either may be None (zero).  `fwd`: what bilstm returned."""
    gates, cell = fwd['gates'], fwd['cell']
    w = [f64(w_hh[0]).to(gates.dtype), f64(w_hh[1]).to(gates.dtype)]
    n, L, _, H4 = gates.shape
    H = H4 // 4
    dh = gates.new_zeros(n, L, 2 * H) if dh is None else f64(dh).to(gates.dtype)
    dc_n = gates.new_zeros(n, 2 * H) if dc_n is None else f64(dc_n).to(gates.dtype)
    dz = torch.zeros_like(gates)
    for s in range(n):
        for d in (0, 1):
            order = list(_steps(int(lens[s]), d == 1))            # the forward pass's order of steps
            dh_rec = gates.new_zeros(H)
            dc = dc_n[s, d * H:(d + 1) * H].clone()
            for k in range(len(order) - 1, -1, -1):
                t = order[k]
                i, f, g, o = gates[s, t, d].split(H)
                c_prev = cell[s, order[k - 1], d] if k > 0 else gates.new_zeros(H)
                tc = torch.tanh(cell[s, t, d])
                dht = dh[s, t, d * H:(d + 1) * H] + dh_rec
                dc = dc + dht * o * (1 - tc * tc)
                dzt = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dht * tc * o * (1 - o)])
                dz[s, t, d] = dzt
                dh_rec = w[d].t() @ dzt
                dc = dc * f
    return dz


def h_before(fwd, lens):
    """h_prev [n, L, 2, H]: the hidden state each step started from (zero at a direction's first step) -- the other operand of dW_hh."""
    h = fwd['h']
    n, L, H2 = h.shape
    H = H2 // 2
    out = h.new_zeros(n, L, 2, H)
    for s in range(n):
        ln = int(lens[s])
        out[s, 1:ln, 0] = h[s, :ln - 1, :H]
        out[s, :ln - 1, 1] = h[s, 1:ln, H:]
    return out


# ---------------------------------------------------------------------------------------------- the kernels' layouts (include/nnr_hip.h)
def p_index(unit, gate):
    """Column of (unit, gate) inside one direction's NP gate columns ("p-order")."""
    return (unit // 16) * 64 + (unit % 16) * 4 + gate


def padded(H):
    """(HP, NP): units and gate columns per direction, padded to whole 16-unit blocks."""
    ub = (H + 15) // 16
    return ub * 16, ub * 64


def gate_columns(H):
    """cols [4H]: p-order column of nn.LSTM's row g*H + unit."""
    unit = torch.arange(H)
    return torch.cat([p_index(unit, g) for g in range(4)])


def length_order(lens):
    """(order, rank): stable descending order of the lengths (sorted position -> sequence) and its inverse (sequence -> sorted position)."""
    order = torch.argsort(torch.as_tensor(lens).long(), descending=True, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(len(order))
    return order, rank


def batch_sizes(lens, L):
    """(bs [L], off [L + 1]): bs[t] = sequences longer than t; off[t] = first packed row of step t, off[L] = number of valid tokens."""
    lens = torch.as_tensor(lens).long()
    bs = torch.stack([(lens > t).sum() for t in range(L)])
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(bs, 0)])
    return bs, off


def packed_row(off, rank, seq, step):
    """Row of (sequence, step) in the packed (time-major, length-sorted) buffers; valid for step < len[seq]."""
    return off[step] + rank[seq]
