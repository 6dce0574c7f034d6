"""Float64 restatement of the GRU user encoder (the reference's userEncoders.py:287-332) in the form the kernels of csrc/gru.hip compute:
every user runs its first len[b] = mask[b].sum() history slots and keeps h from then on.  tests/test_gru_host.py pins it to torch.nn.GRU on a
PackedSequence through the reference's sort / drop-empties / de-sort path; the GPU tests compare the kernels with it."""
import torch
from torch.nn.utils.rnn import pack_padded_sequence


def f64(t):
    return (t if torch.is_tensor(t) else torch.as_tensor(t)).detach().cpu().double()


def lengths(mask):
    """pack_padded_sequence semantics: only the COUNT of ones matters, not where they sit."""
    return (f64(mask) != 0).sum(dim=1)


def gru_frozen(x, lens, w_ih, w_hh, b_ih, b_hh, h0=None):
    """x [B, T, D], lens [B] -> (hs [B, T, H] with h_t at the live slots and zero elsewhere, h_final [B, H]).  torch's nn.GRU cell, gate
    order r | z | n; b_hn sits inside the reset gate's product."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros((B, H)) if h0 is None else h0
    hs = []
    for t in range(T):
        gx = x[:, t] @ w_ih.t() + b_ih
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gx[:, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
        live = (t < lens).to(x.dtype).unsqueeze(1)
        h = live * ((1 - z) * n + z * h) + (1 - live) * h
        hs.append(h * live)
    return torch.stack(hs, dim=1), h


def packed_path(x, mask, gru, h0=None):
    """h_final [B, H] along the reference's own path (userEncoders.py:304-329): sort by length, drop the empty users, pack, nn.GRU, put zero
    rows (h0 rows when a start state is given) back, de-sort.  `gru`: a torch.nn.GRU(batch_first=True) in float64."""
    B = x.shape[0]
    num = lengths(mask).long()
    snum, sidx = torch.sort(num, descending=True)
    _, desort = torch.sort(sidx, descending=False)
    H = gru.hidden_size
    rest = x.new_zeros((B, H)) if h0 is None else h0.index_select(0, sidx)
    live = int((snum > 0).sum())
    if live == 0:
        return rest.index_select(0, desort)
    keep = sidx[:live]
    packed = pack_padded_sequence(x.index_select(0, keep), snum[:live].cpu(), batch_first=True)
    start = None if h0 is None else h0.index_select(0, keep).unsqueeze(0)
    _, h = gru(packed, start)
    return torch.cat([h.squeeze(0), rest[live:]], dim=0).index_select(0, desort)


def gru_user_rep(hist, mask, state, prefix='user_encoder.'):
    """The user vector [B, D]: tanh(dec(h_final)), exactly zero for a user without history.  state: {name: array} of the encoder's parameters."""
    p = {k: f64(state[prefix + k]) for k in ('gru.weight_ih_l0', 'gru.weight_hh_l0', 'gru.bias_ih_l0', 'gru.bias_hh_l0', 'dec.weight', 'dec.bias')}
    lens = lengths(mask)
    _, h = gru_frozen(f64(hist), lens, p['gru.weight_ih_l0'], p['gru.weight_hh_l0'], p['gru.bias_ih_l0'], p['gru.bias_hh_l0'])
    return torch.tanh(h @ p['dec.weight'].t() + p['dec.bias']) * (lens > 0).double().unsqueeze(1)


def prefix_mask(lens, T):
    return torch.arange(T).unsqueeze(0) < torch.as_tensor(lens).unsqueeze(1)


# ---------------------------------------------------------------------------------------------- the packed layouts, read back
def p_index(unit, slot):
    return (unit // 16) * 64 + (unit % 16) * 4 + slot


def unpack_forward_fragments(wf, H):
    """wf [UB][3][KG][64 lanes][4] -> W_hh [3H, H] (nnr_hip.h: wf[ub][g][kg][lane][ii] = w_hh[g*H + ub*16 + (lane & 15)][16 kg + 4 (lane >> 4) + ii])."""
    UB = (H + 15) // 16
    w = wf.view(UB, 3, UB, 4, 16, 4)                     # ub, g, kg, lane >> 4, lane & 15, ii
    full = w.permute(1, 0, 4, 2, 3, 5).reshape(3, UB * 16, UB * 16)
    return full[:, :H, :H].reshape(3 * H, H), full


def unpack_backward_fragments(wb, H):
    """wb [UB][NP/16][64 lanes][4] -> W_hh [3H, H] (wb[ubn][kg][lane][ii] = row p = 16 kg + 4 (lane >> 4) + ii of the p-ordered W_hh, column
    ubn*16 + (lane & 15); slot 2 rows are zero, slot 3 rows are the n gate's)."""
    UB = (H + 15) // 16
    NP = UB * 64
    w = wb.view(UB, NP // 16, 4, 16, 4)                  # ubn, kg, lane >> 4, lane & 15, ii
    rows = w.permute(1, 2, 4, 0, 3).reshape(NP, UB * 16)  # [p][col]
    unit = torch.arange(H)
    out = torch.cat([rows[p_index(unit, s)][:, :H] for s in (0, 1, 3)], dim=0)
    return out, rows
