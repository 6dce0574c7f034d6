"""float64 restatement of the masked-softmax attention pool (nnr_amd/csrc/pool.hip) in plain torch on the CPU, the packing helpers of the
time-major packed layout, a restatement of the kernel's dispatch, and the case tables that tests/test_hip_pool_gpu.py runs and
tests/test_pool_host.py checks for coverage of every path.

  pool_ref     alpha, out, dx, dscore, dv through autograd of oracle.nnr_oracle.masked_softmax's semantics: where(mask, s, -1e9), then
               softmax over t < len
  path_of      which kernel instantiation and which body a sequence takes (follows pool_launch / pool_packed_kernel)
  packed_rows, pack, unpack     rows = off[t] + rank[i]"""
import types

import torch

# ------------------------------------------------------------------------------------------------ the kernel's constants (csrc/pool.hip)
MAX_D = 1280            # 4 * 64 * MAXV_ALL
MAX_L = 128             # 64 * MAXT
MAX_A = 256             # the fused th . w2 score: one float4 per lane
PACKED_MAX_D = 512      # pool_launch: the register-resident packed kernels hold nv <= 128 float4 per row
TEAM_R = 8              # rows per wave: single-wave teams up to R tokens, four-wave teams up to 4 R, the stream body beyond

INSTANTIATIONS = ('packed NV1', 'packed NV2', 'pool_kernel NV1', 'pool_kernel NV2', 'pool_kernel NV4', 'pool_kernel NV5')
BODIES = ('single', 'team', 'stream')


def path_of(packed, D, L, length):
    """(instantiation, body) of one sequence of `length` tokens in a call with row width D and maximal length L.  This restates
    pool_launch and pool_packed_kernel and MUST FOLLOW THE KERNEL'S CONSTANTS (R = 8 rows per wave, nv <= 64 / 128 / 256 float4 per
    row, the packed kernels up to D = 512 and L = 128): a change there that is not made here voids the coverage assertion of
    tests/test_pool_host.py.  A dense call has no lengths: every sequence takes the stream body with `length` = L."""
    assert D % 4 == 0 and 0 < D <= MAX_D and 0 < L <= MAX_L and 0 < length <= L
    nv = D // 4
    if packed and D <= PACKED_MAX_D and L <= MAX_L:
        inst = 'packed NV1' if nv <= 64 else 'packed NV2'
        # nstream = L > 4 R ? bs[4 R] : 0 sequences come first (sorted by descending length), then ncoop = L > R ? bs[R] : 0
        if L > 4 * TEAM_R and length > 4 * TEAM_R:
            return inst, 'stream'
        if L > TEAM_R and length > TEAM_R:
            return inst, 'team'
        return inst, 'single'
    inst = 'pool_kernel NV%d' % (1 if nv <= 64 else 2 if nv <= 128 else 4 if nv <= 256 else 5)
    return inst, 'stream'


def short_count(packed, D, L, lens):
    """Sequences served by single-wave teams, four per workgroup (None when the call does not run the packed kernels)."""
    if not (packed and D <= PACKED_MAX_D):
        return None
    return sum(1 for l in lens if path_of(True, D, L, l)[1] == 'single')


# ------------------------------------------------------------------------------------------------ the reference
def pool_ref(x, lens=None, score=None, v=None, scale=1.0, th=None, w2=None, mask=None, mask_div=1, add_in=None, dout=None, dout2=None,
             v_b=None, scale_b=1.0, dout_b=None):
    """x [n, L, D]; lens [n] or None (dense: every sequence has L tokens); the score is `score` [n, L] (GIVEN), scale * <x, v> with
    v [n, D] (DOT), or <th, w2> with th [n, L, A], w2 [A] (the fused row-dot; th is an input of its own, no gradient reaches x through
    it); mask [n / mask_div, L], 0 = masked; out = sum_t alpha_t x_t (+ add_in).  With dout [n, D] (+ dout2) the gradients of
    sum(out * (dout + dout2)): dx, dscore (of the score BEFORE the mask replaced it) and dv.  With v_b / scale_b / dout_b a second
    pool (DOT) over the same x is added to the loss, sum(out_b * dout_b): dx is then the gradient of both, and alpha_b, out_b,
    dscore_b, dv_b are returned too.  Everything float64."""
    n, L, D = x.shape
    f64 = torch.float64
    xr = x.detach().to(f64).clone().requires_grad_(True)
    live = torch.ones(n, L, dtype=torch.bool) if lens is None else torch.arange(L)[None, :] < torch.as_tensor(lens).long()[:, None]
    keep = None
    if mask is not None:
        keep = mask.bool().repeat_interleave(mask_div, dim=0)
        assert keep.shape == (n, L)

    def softmax_pool(s):
        if keep is not None:
            s = torch.where(keep, s, torch.full_like(s, -1e9))               # oracle.nnr_oracle.masked_softmax
        s = torch.where(live, s, torch.full_like(s, float('-inf')))          # positions beyond the length do not exist
        alpha = torch.softmax(s, dim=1)
        return alpha, torch.einsum('nl,nld->nd', alpha, xr)

    r = types.SimpleNamespace(live=live)
    vr = None
    if v is not None:
        vr = v.detach().to(f64).clone().requires_grad_(True)
        s = scale * torch.einsum('nld,nd->nl', xr, vr)
    elif th is not None:
        s = torch.einsum('nla,a->nl', th.detach().to(f64), w2.detach().to(f64).reshape(-1)).requires_grad_(True)
    else:
        s = score.detach().to(f64).clone().requires_grad_(True)
    if not s.is_leaf:
        s.retain_grad()
    alpha, out = softmax_pool(s)
    r.score, r.alpha = s.detach(), alpha.detach()
    r.out = out.detach() + (add_in.to(f64) if add_in is not None else 0.0)
    vbr = None
    if v_b is not None:
        vbr = v_b.detach().to(f64).clone().requires_grad_(True)
        s_b = scale_b * torch.einsum('nld,nd->nl', xr, vbr)
        s_b.retain_grad()
        alpha_b, out_b = softmax_pool(s_b)
        r.alpha_b, r.out_b = alpha_b.detach(), out_b.detach()
    if dout is None:
        return r
    g = dout.to(f64) + (dout2.to(f64) if dout2 is not None else 0.0)
    loss = (out * g).sum()
    if v_b is not None:
        loss = loss + (out_b * dout_b.to(f64)).sum()
    loss.backward()
    r.dx, r.dscore = xr.grad, s.grad
    r.dv = vr.grad if vr is not None else None
    if v_b is not None:
        r.dscore_b, r.dv_b = s_b.grad, vbr.grad
    return r


# ------------------------------------------------------------------------------------------------ the packed layout
def packed_rows(off, rank, L):
    """[n, L] int64: the packed row of position t of the caller's sequence i, off[t] + rank[i] (meaningful where t < len[i])."""
    return off.cpu().long()[:L][None, :] + rank.cpu().long()[:, None]


def pack(dense, rows, live, cap, ld=None, fill=float('nan')):
    """[n, L] or [n, L, C] -> [cap] or [cap, ld]: the live positions at their packed rows, `fill` everywhere else (rows at or beyond the
    plan's total, and the columns C .. ld of every row)."""
    if dense.dim() == 2:
        out = torch.full((cap,), fill, dtype=dense.dtype)
        out[rows[live]] = dense[live]
        return out
    C_ = dense.shape[2]
    out = torch.full((cap, ld or C_), fill, dtype=dense.dtype)
    out[rows[live], :C_] = dense[live]
    return out


def unpack(packed, rows, live, C_=None, fill=0.0):
    """The inverse of pack: [cap] or [cap, ld] -> [n, L] or [n, L, C_] with `fill` at the positions that do not exist."""
    packed = packed.detach().cpu()
    n, L = rows.shape
    if packed.dim() == 1:
        out = torch.full((n, L), fill, dtype=packed.dtype)
        out[live] = packed[rows[live]]
        return out
    C_ = C_ or packed.shape[1]
    out = torch.full((n, L, C_), fill, dtype=packed.dtype)
    out[live] = packed[rows[live], :C_]
    return out


# ------------------------------------------------------------------------------------------------ case tables (shared by both test files)
LADDER = [128, 127, 65, 64, 63, 37, 36, 33, 32, 31, 17, 12, 9, 8, 8, 5, 2, 1, 1]
LENGTH_TABLES = {                                   # name -> (L, lengths)
    'ladder': (128, LADDER),                        # six short sequences: the last workgroup of single-wave teams is half filled
    'ladder-1': (128, LADDER[:-1]),                 # five
    'ladder-3': (128, LADDER[:-3]),                 # three
    'short_only': (8, [8, 1, 5, 3, 8, 2, 7]),       # L <= 8: no team, no stream
    'short_in_L12': (12, [8, 7, 3, 1, 8, 4]),       # L > 8, but no sequence longer than 8
    'no_short': (40, [40, 33, 32, 9, 20]),
    'mid': (32, [32, 9, 8, 1]),
    'one_long': (128, [128]),
    'one_short': (1, [1]),
}
MODES = ('given', 'dot', 'th')
TH_A = 200


def table_lens(name):
    """(L, lengths in the caller's row order): the table through a fixed permutation, so that the plan's `order` is not the identity."""
    L, lens = LENGTH_TABLES[name]
    n = len(lens)
    perm = [(5 * i + 3) % n for i in range(n)] if n % 5 else [(3 * i + 1) % n for i in range(n)]
    assert sorted(perm) == list(range(n))
    return L, [lens[p] for p in perm]


def packed_cases():
    """(table, D, mode, A, ldth): `ladder` at every D class in every mode (+ A = 4 and A = 256 with ldth > A at D = 260), every other
    table at D = 260."""
    cases = [('ladder', D, m, TH_A if m == 'th' else 0, TH_A if m == 'th' else 0) for D in (4, 256, 260, 512, 516, 1280) for m in MODES]
    cases += [('ladder', 260, 'th', 4, 12), ('ladder', 260, 'th', 256, 264)]
    cases += [(t, 260, m, TH_A if m == 'th' else 0, TH_A if m == 'th' else 0) for t in LENGTH_TABLES if t != 'ladder' for m in MODES]
    return cases


HOLE_CASES = [(L, D, m) for L in (8, 20, 70) for D in (256, 260) for m in MODES]          # n = HOLE_N rows, see hole_mask
HOLE_N = 9
DENSE_SHAPES = [(3, 1, 4), (4, 64, 256), (3, 65, 260), (6, 50, 400), (5, 19, 900), (2, 128, 1028), (2, 128, 1280)]
DENSE_TH_SHAPES = [(4, 64, 256), (3, 65, 260)]
DENSE_MASKS = ('none', 'div1', 'div3')              # div3 on n = 6 only: two groups of three share a mask row


def dense_cases():
    out = []
    for (n, L, D) in DENSE_SHAPES:
        for m in MODES:
            if m == 'th' and (n, L, D) not in DENSE_TH_SHAPES:
                continue
            for mk in DENSE_MASKS:
                if mk == 'div3' and n != 6:
                    continue
                out.append((n, L, D, m, mk))
    return out


FOLD_CASES = [(t, D) for t in ('ladder', 'mid') for D in (256, 260, 516)]
STRIDE_CASES = [('ladder', 256), ('ladder', 260), ('ladder', 516), ('dense', 260)]          # dense: (3, 65, 260)
STRIDE_DENSE = (3, 65, 260)


def hole_mask(n, L, seed):
    """[n, L] bool: row 0 fully masked, row 1 fully live, row 2 with only the last position live, row 3 with only position 0 live, the
    rest random with holes and at least one live position (rows that do not exist are left out, and at L = 1 the kinds coincide)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, L, generator=g) < 0.6
    first = torch.randint(0, L, (n,), generator=g)
    m[torch.arange(n), first] = True
    if L > 2:
        for i in range(4, n):                      # a hole for certain
            m[i, (int(first[i]) + 1) % L] = False
    m[0] = False
    if n > 1:
        m[1] = True
    if n > 2:
        m[2] = False
        m[2, L - 1] = True
    if n > 3:
        m[3] = False
        m[3, 0] = True
    return m


def cover_lens(mask):
    """Length of every row under ops.mask_cover: up to the last live position, all L positions for a row without one."""
    n, L = mask.shape
    last = (mask.long() * torch.arange(1, L + 1)[None, :]).max(dim=1).values
    return torch.where(last > 0, last, torch.full_like(last, L)).tolist()
