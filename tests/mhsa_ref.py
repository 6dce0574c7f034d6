"""Float64 restatement of the MHSA attention core (layers.py:137-147 after the projections), Python restatements of the host-side rules
around it (the persistent backward's groups-per-workgroup rule, the paired-title layout), and the case tables shared by
tests/test_mhsa_host.py (CPU) and tests/test_hip_mhsa_gpu.py (MI355X).  Plain torch on the CPU; nothing here touches the HIP library."""
import functools
import math
from types import SimpleNamespace

import torch

BAR = 2e-5            # the project's op-level bar (close() in tests/test_hip_ops_gpu.py): |got - ref| <= BAR * max(1, max|ref|)
JUNK = 77.0           # dense rows that do not exist in the packed form (masked keys must make them irrelevant)
DROP = (0.2, 1234)    # (p, seed) of the fused-dropout checks


# ------------------------------------------------------------------------------------------------ reference
def attention_ref(qkv, mask, n, Lq, heads, dh):
    """qkv [n*Lq, 3*heads*dh] -> out [n*Lq, heads*dh] in float64: scores / sqrt(dh), masked keys at -1e9 (mask None: no masking; a fully
    masked sample therefore gets the uniform softmax), softmax over keys, P V.  Differentiable in qkv."""
    HD = heads * dh
    x = qkv if qkv.dtype == torch.float64 else qkv.double()
    q, k, v = (x[:, s * HD:(s + 1) * HD].reshape(n, Lq, heads, dh) for s in range(3))
    s_ = torch.einsum('nqhd,nkhd->nhqk', q, k) / math.sqrt(dh)
    if mask is not None:
        s_ = torch.where(mask.bool()[:, None, None, :], s_, torch.full_like(s_, -1e9))
    return torch.einsum('nhqk,nkhd->nqhd', torch.softmax(s_, 3), v).reshape(n * Lq, HD)


def group_plan(heads, n):
    """(ngroups, gp) of the persistent backward (mhsa_bwd_launch): 4-head groups, and how many consecutive groups one workgroup walks --
    a sample's worth, or fewer while that leaves fewer than 1024 workgroups."""
    ngroups = n * heads // 4
    gp = heads // 4
    while gp > 1 and (ngroups + gp - 1) // gp < 1024:
        gp -= 1
    return ngroups, gp


def dispatch(Lq, heads, dh, saved_prob):
    """(forward, backward) kernel instantiation that mhsa_fwd_launch / mhsa_bwd_launch select, and whether each runs the cooperative
    4-head staging -- the table of csrc/mhsa.hip's dispatcher, restated so that the suite can say which of the twelve a case reaches."""
    nb = 2 if Lq > 32 else 1
    d = 20 if dh == 20 else 0
    coop_f = heads % 4 == 0 and dh % 4 == 0
    fwd = 'fwd<%d,%d%s>' % (nb, d, ',FULL' if nb == 1 and dh == 20 and Lq == 32 else '')
    coop_b = nb == 1 and coop_f
    if coop_b and not saved_prob and 32 * dh <= 768:
        bwd = 'persist<%d,%s>' % (d, 'true' if dh == 20 and Lq == 32 else 'false')
    else:
        bwd = 'bwd<%d,%d>' % (nb, d)
    return (fwd, coop_f), (bwd, coop_b)


INSTANTIATIONS = ['fwd<1,20,FULL>', 'fwd<1,20>', 'fwd<1,0>', 'fwd<2,20>', 'fwd<2,0>', 'persist<20,true>', 'persist<20,false>', 'persist<0,false>',
                  'bwd<1,20>', 'bwd<1,0>', 'bwd<2,20>', 'bwd<2,0>']


def pair_layout(cover_lens_sorted):
    """Restatement of mhsa_pairing / mhsa_pair_map_kernel over the plan's sorted (descending) cover lengths: titles covering more than 16
    positions stay alone, those covering 9..16 go two to a virtual sample (slots 0 / 16), the rest four (slots 0 / 8 / 16 / 24).
    members[v] = [(sorted position, first slot), ...]; width = positions per slot of that virtual sample."""
    sl = [int(x) for x in cover_lens_sorted]
    n = len(sl)
    assert all(a >= b for a, b in zip(sl, sl[1:])) and all(1 <= x <= 32 for x in sl)
    n16 = sum(1 for x in sl if x > 16)
    n8 = sum(1 for x in sl if x > 8)
    np_ = (n8 - n16 + 1) // 2
    nq = (n - n8 + 3) // 4
    members, width = [], []
    for v in range(n16):
        members.append([(v, 0)])
        width.append(32)
    for k in range(np_):
        members.append([(s, 16 * j) for j, s in enumerate(range(n16 + 2 * k, min(n8, n16 + 2 * k + 2)))])
        width.append(16)
    for k in range(nq):
        members.append([(s, 8 * j) for j, s in enumerate(range(n8 + 4 * k, min(n, n8 + 4 * k + 4)))])
        width.append(8)
    return SimpleNamespace(n=n, n16=n16, n8=n8, np=np_, nv=n16 + np_ + nq, members=members, width=width)


def cover_ref(mask):
    """ops.mask_cover on the CPU: every position up to the last live one; all positions of a title without a live one."""
    n, L = mask.shape
    pos = torch.arange(L)[None, :]
    last = torch.where(mask.bool(), pos, torch.full_like(pos, -1)).max(1).values
    last = torch.where(last < 0, torch.full_like(last, L - 1), last)
    return pos <= last[:, None]


def plan_ref(cover):
    """The planner's outputs that the attention core uses, on the CPU: order (stable, descending length), slen, off [L + 1]."""
    n, L = cover.shape
    lens = cover.sum(1)
    order = torch.sort(lens, descending=True, stable=True).indices
    slen = lens[order]
    bs = (lens[None, :] > torch.arange(L)[:, None]).sum(1)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(bs, 0)])
    return order, slen, off


def pair_maps(layout, off, slen, order, mask):
    """(vrowmap, vmask) [n, 32] that nnr_mhsa_pair_map must produce for `layout`: packed row off[t] + s of position t < slen[s] of the
    title at sorted position s, the ORIGINAL mask of every position of its slot; (-1, 0) everywhere else."""
    n = layout.n
    vrow = torch.full((n, 32), -1, dtype=torch.int32)
    vmask = torch.zeros((n, 32), dtype=torch.uint8)
    for v, (mem, w) in enumerate(zip(layout.members, layout.width)):
        for s, slot in mem:
            for t in range(w):
                if t < int(slen[s]):
                    vrow[v, slot + t] = int(off[t]) + s
                vmask[v, slot + t] = int(mask[int(order[s]), t])
    return vrow, vmask


# ------------------------------------------------------------------------------------------------ inputs
def _randn(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def make_masks(n, Lq, kind, seed):
    """`none`: None.  `random`: 70 % live.  `edges`: sample 0 fully masked, 1 all live, 2 only the last key live, 3 only key 0 live, 4 with
    an interior gap (where Lq >= 3), the rest random; a batch of fewer than 5 samples takes the first n of these."""
    if kind == 'none':
        return None
    mask = torch.rand(n, Lq, generator=torch.Generator().manual_seed(seed)) < 0.7
    if kind == 'random':
        return mask
    assert kind == 'edges'
    rows = [torch.zeros(Lq, dtype=torch.bool), torch.ones(Lq, dtype=torch.bool), torch.arange(Lq) == Lq - 1, torch.arange(Lq) == 0,
            torch.ones(Lq, dtype=torch.bool)]
    if Lq >= 3:
        rows[4][Lq // 2] = False
    for i, r in enumerate(rows[:n]):
        mask[i] = r
    return mask


def _case(kind, tag, n, Lq, heads, dh, mask, seed, cover=None, scale=0.7, **extra):
    """qkv = randn * scale (0.7 unless TUNED says otherwise), dout = randn, both from seeded CPU generators.  With `cover` (packed /
    paired cases) the dense restatement holds JUNK in the qkv rows that the packed form does not have, and no upstream gradient there."""
    HD = heads * dh
    qkv = _randn((n * Lq, 3 * HD), seed, scale)
    dout = _randn((n * Lq, HD), seed + 1)
    if cover is not None:
        dead = ~cover.reshape(-1)
        qkv[dead] = JUNK
        dout[dead] = 0.0
    return SimpleNamespace(kind=kind, tag=tag, scale=scale, n=n, Lq=Lq, heads=heads, dh=dh, mask=mask, cover=cover, qkv=qkv, dout=dout, **extra)


# (n, Lq, heads, dh): what it pins
DENSE_SHAPES = [
    (5, 32, 8, 20),      # fwd<1,20,FULL> coop; bwd persist<20,true> / bwd<1,20> with prob
    (5, 31, 8, 20),      # fwd<1,20>; persist<20,false>; the last query and key row exactly at the `< Lq` predicate
    (5, 1, 4, 20),       # softmax over a single key
    (5, 32, 6, 20),      # heads % 4 != 0: one head per wave, float4 staging; n*heads % 4 != 0: the last workgroup has idle waves
    (5, 33, 8, 20),      # first length on NB = 2; bwd<2,20>
    (5, 64, 4, 20),      # NB = 2 with no padded position
    (5, 64, 4, 32),      # <2,0> forward and backward at the largest dh
    (5, 63, 3, 30),      # NB = 2, dh % 4 != 0: scalar staging
    (5, 32, 4, 32),      # fwd<1,0> coop; backward without prob is bwd<1,0> with coop = 1 (32*dh > 768)
    (5, 17, 4, 28),      # the same with Lq < 32
    (5, 32, 4, 24),      # persist<0,false> at its limit 32*dh == 768
    (6, 9, 4, 4),        # persist<0,false> at the smallest dh on the float4 path
    (7, 20, 5, 6),       # one head per wave, scalar staging, NB = 1
    (5, 2, 1, 2),        # the smallest of everything
]
DENSE_KINDS = ['none', 'edges']
# the persistent backward's group loop: the smallest shapes that make it iterate (gp > 1 needs n*heads/4 >= 2048)
GROUP_LOOP_SHAPES = [
    (701, 32, 12, 20),   # persist<20,true>; 2103 groups, gp = 2: workgroups straddle samples, the last one holds one group
    (701, 8, 12, 4),     # persist<0,false>, the same plan
    (1025, 8, 8, 20),    # persist<20,false>; 2050 groups, gp = 2 = heads/4: every workgroup is one sample's two groups
]
PACKED_SHAPES = [(40, 32, 8, 20), (40, 20, 4, 20), (40, 32, 4, 8), (40, 32, 4, 28), (40, 12, 4, 32)]
PACKED_PROFILES = ['random', 'full', 'one', 'edges']
PAIRED_DHS = [20, 4, 24]
PAIRED_PROFILES = ['mixed', 'long', 'pairs7', 'quad5', 'quad6', 'quad7', 'single', 'long_short', 'bounds', 'masked_mix']
PAIRED_GROUP_LOOP = ('mixed', 701, 12, 20)      # the paired path with gp > 1: the device-side group count follows nv, the grid follows n


# case key -> (seed salt, qkv scale) where the default (0, 0.7) misses the input-magnitude condition of tests/test_mhsa_host.py (small
# slices: a fully masked sample's output is the MEAN of its values, ~scale / sqrt(Lq); a two-key softmax at dh = 2 has hardly any
# gradient).  Found by walking salts 0.. and scales 0.7, 1.0, 1.4 on the CPU reference alone; no kernel result went into them.
TUNED = {
    ('dense', 5, 32, 8, 20, 'edges'): (0, 1.0), ('dense', 5, 31, 8, 20, 'edges'): (3, 0.7), ('dense', 5, 32, 6, 20, 'edges'): (3, 0.7),
    ('dense', 5, 64, 4, 20, 'none'): (0, 1.0), ('dense', 5, 64, 4, 20, 'edges'): (1, 1.0), ('dense', 5, 64, 4, 32, 'none'): (0, 1.0),
    ('dense', 5, 64, 4, 32, 'edges'): (1, 1.0), ('dense', 5, 63, 3, 30, 'none'): (0, 1.0), ('dense', 5, 63, 3, 30, 'edges'): (1, 1.0),
    ('dense', 6, 9, 4, 4, 'none'): (0, 1.0), ('dense', 6, 9, 4, 4, 'edges'): (4, 0.7), ('dense', 7, 20, 5, 6, 'none'): (3, 0.7),
    ('dense', 7, 20, 5, 6, 'edges'): (1, 0.7), ('dense', 5, 2, 1, 2, 'none'): (15, 1.4), ('dense', 5, 2, 1, 2, 'edges'): (3, 1.4),
    ('loop', 701, 8, 12, 4): (0, 1.0),
    ('packed', 40, 20, 4, 20, 'edges'): (1, 0.7), ('packed', 40, 32, 4, 8, 'full'): (0, 1.0), ('packed', 40, 32, 4, 8, 'edges'): (2, 0.7),
    ('paired', 'quad5', 4, 20, None): (2, 0.7), ('paired', 'long_short', 4, 20, None): (1, 0.7), ('paired', 'masked_mix', 4, 20, None): (1, 0.7),
    ('paired', 'mixed', 4, 4, None): (0, 1.0), ('paired', 'long', 4, 4, None): (0, 1.0), ('paired', 'pairs7', 4, 4, None): (0, 1.0),
    ('paired', 'quad5', 4, 4, None): (3, 1.0), ('paired', 'quad6', 4, 4, None): (2, 1.0), ('paired', 'quad7', 4, 4, None): (4, 0.7),
    ('paired', 'single', 4, 4, None): (1, 0.7), ('paired', 'long_short', 4, 4, None): (3, 1.0), ('paired', 'bounds', 4, 4, None): (0, 1.0),
    ('paired', 'masked_mix', 4, 4, None): (2, 1.0), ('paired', 'quad5', 4, 24, None): (2, 0.7), ('paired', 'quad6', 4, 24, None): (1, 0.7),
    ('paired', 'quad7', 4, 24, None): (1, 0.7), ('paired', 'masked_mix', 4, 24, None): (1, 0.7), ('paired', 'mixed', 12, 20, 701): (3, 1.0),
}


def _seed(*key):
    """(seed, qkv scale) of a case: a stable hash of its key (python's hash() of a str is salted per process) plus the case's salt, and
    the case's scale, both from TUNED where the default (0, 0.7) does not meet the input-magnitude condition."""
    salt, scale = TUNED.get(key, (0, 0.7))
    h = 0
    for c in repr(key):
        h = (h * 131 + ord(c)) % 1000003
    return h + 7919 * salt, scale


@functools.lru_cache(maxsize=2)
def dense_case(n, Lq, heads, dh, kind):
    seed, scale = _seed('dense', n, Lq, heads, dh, kind)
    return _case('dense', 'dense n%d L%d h%d d%d %s' % (n, Lq, heads, dh, kind), n, Lq, heads, dh, make_masks(n, Lq, kind, seed + 2), seed, scale=scale)


@functools.lru_cache(maxsize=2)
def group_loop_case(n, Lq, heads, dh):
    seed, scale = _seed('loop', n, Lq, heads, dh)
    mask = make_masks(n, Lq, 'random', seed + 2)
    mask[0] = False
    return _case('dense', 'loop n%d L%d h%d d%d' % (n, Lq, heads, dh), n, Lq, heads, dh, mask, seed, scale=scale)


def _prefix(lens, L):
    return torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]


@functools.lru_cache(maxsize=2)
def packed_case(n, L, heads, dh, profile):
    seed, scale = _seed('packed', n, L, heads, dh, profile)
    g = torch.Generator().manual_seed(seed + 2)
    if profile == 'full':
        lens = torch.full((n,), L)
    elif profile == 'one':
        lens = torch.ones(n, dtype=torch.long)
    else:
        lens = torch.randint(1, L + 1, (n,), generator=g)
    mask = _prefix(lens, L)
    if profile == 'edges':
        mask[5] = False              # fully masked: uniform softmax, all L positions are rows
        mask[9, :6] = True           # an interior masked position: a row that exists but is masked
        mask[9, 3] = False
    return _case('packed', 'packed n%d L%d h%d d%d %s' % (n, L, heads, dh, profile), n, L, heads, dh, mask, seed, cover=cover_ref(mask), scale=scale)


def paired_lengths(profile, n=None, seed=0):
    """Cover lengths (in the caller's row order, shuffled so that the plan's order is no identity) of a paired-title profile."""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi, k):
        return torch.randint(lo, hi + 1, (k,), generator=g).tolist()
    if profile == 'mixed':           # n16 < n8 < n
        n = n or 45
        a, b = n // 3, n // 3
        lens = ri(17, 32, a) + ri(9, 16, b) + ri(1, 8, n - a - b)
    elif profile == 'long':          # nv == n, nothing grouped
        lens = ri(17, 32, 6)
    elif profile == 'pairs7':        # an incomplete pair
        lens = ri(9, 16, 7)
    elif profile in ('quad5', 'quad6', 'quad7'):      # an incomplete quad of 1, 2, 3 titles
        lens = ri(1, 8, int(profile[-1]))
    elif profile == 'single':
        lens = [5]
    elif profile == 'long_short':
        lens = [32, 3]
    elif profile == 'bounds':
        lens = [8, 9, 16, 17] * 2
    elif profile == 'masked_mix':    # row 0 becomes the fully masked title, row 1 the title whose only live key is its last position
        lens = [32, 5] + ri(17, 32, 2) + ri(9, 16, 4) + ri(1, 8, 5)
        return lens                  # (not shuffled: rows 0 and 1 are rewritten by the case builder)
    else:
        raise KeyError(profile)
    perm = torch.randperm(len(lens), generator=g).tolist()
    return [lens[i] for i in perm]


@functools.lru_cache(maxsize=2)
def paired_case(profile, heads, dh, n=None):
    seed, scale = _seed('paired', profile, heads, dh, n)
    lens = paired_lengths(profile, n, seed + 2)
    mask = _prefix(lens, 32)
    if profile == 'masked_mix':
        mask[0] = False              # covers all 32 positions and must stay alone
        mask[1] = False
        mask[1, 4] = True            # covers 5 positions, only the last one live
    cover = cover_ref(mask)
    assert cover.sum(1).tolist() == list(lens)
    return _case('paired', 'paired %s n%d h%d d%d' % (profile, len(lens), heads, dh), len(lens), 32, heads, dh, mask, seed, cover=cover, scale=scale)


def case_key(builder, args):
    """The TUNED key of a case of all_cases()."""
    kind = {'dense_case': 'dense', 'group_loop_case': 'loop', 'packed_case': 'packed', 'paired_case': 'paired'}[builder.__wrapped__.__name__]
    args = tuple(args)
    return (kind,) + (args + (None,) if kind == 'paired' and len(args) == 3 else args)


def all_cases():
    """Every case of the GPU suite as (builder, args): what the input-magnitude condition of tests/test_mhsa_host.py walks."""
    out = [(dense_case, s + (k,)) for s in DENSE_SHAPES for k in DENSE_KINDS]
    out += [(group_loop_case, s) for s in GROUP_LOOP_SHAPES]
    out += [(packed_case, s + (p,)) for s in PACKED_SHAPES for p in PACKED_PROFILES]
    out += [(paired_case, (p, 4, dh)) for dh in PAIRED_DHS for p in PAIRED_PROFILES]
    out += [(paired_case, (PAIRED_GROUP_LOOP[0], PAIRED_GROUP_LOOP[2], PAIRED_GROUP_LOOP[3], PAIRED_GROUP_LOOP[1]))]
    return out


def reference(case, dout=None):
    """(out, dqkv) in float64 for the case's inputs (dout: another upstream gradient than the case's)."""
    x = case.qkv.double().requires_grad_(True)
    out = attention_ref(x, case.mask, case.n, case.Lq, case.heads, case.dh)
    (out * (case.dout if dout is None else dout).double()).sum().backward()
    return out.detach(), x.grad


def slice_health(case):
    """max|ref| of every (sample, head) slice of out, dV, dQ, dK for the input-magnitude condition (tests/test_mhsa_host.py), and the
    largest |dQ|, |dK| of the samples exempt from it: those with at most ONE live key -- fully masked (the -1e9 constant passes no
    gradient) or one live key (P is one-hot, so dS = P (dP - delta) is exactly zero: every sample of an Lq == 1 case, every title of one
    position, the one-key rows of the `edges` masks)."""
    n, Lq, heads, dh = case.n, case.Lq, case.heads, case.dh
    out, dqkv = reference(case)
    nlive = torch.full((n,), Lq) if case.mask is None else case.mask.sum(1)
    graded = nlive >= 2
    mo = slice_max(out, n, Lq, heads, dh, 1, case.cover)[:, 0]                  # [n, heads]
    mg = slice_max(dqkv, n, Lq, heads, dh, 3, case.cover)                       # [n, 3, heads]
    exempt = float(mg[~graded, :2].max()) if bool((~graded).any()) else 0.0
    return {'out': mo, 'dV': mg[:, 2], 'dQ': mg[graded, 0], 'dK': mg[graded, 1]}, exempt


# ------------------------------------------------------------------------------------------------ the bar, slice by slice
def _slices(t, n, Lq, heads, dh, nmat):
    return t.detach().double().cpu().reshape(n, Lq, nmat, heads, dh)


def slice_max(ref, n, Lq, heads, dh, nmat, live=None):
    """max|ref| of every (sample, matrix, head) slice [n, nmat, heads]; `live` [n, Lq]: only these positions count."""
    r = _slices(ref, n, Lq, heads, dh, nmat).abs()
    if live is not None:
        r = r * live.reshape(n, Lq, 1, 1, 1).double()
    return r.amax(dim=(1, 4))


def slice_bar(got, ref, n, Lq, heads, dh, nmat, live=None, what=''):
    """The project's bar |got - ref| <= 2e-5 * max(1, max|ref|), with max|ref| taken over each (sample, head, matrix) slice
    ([Lq, dh] of got / ref [n*Lq, nmat*heads*dh]) instead of the whole tensor.  `live` [n, Lq] bool: positions outside it are not rows of
    the packed form and are left out of both sides.  Returns the largest error / bar; a NaN in a compared position fails."""
    g, r = _slices(got, n, Lq, heads, dh, nmat), _slices(ref, n, Lq, heads, dh, nmat)
    err = (g - r).abs()
    if live is not None:
        keep = live.reshape(n, Lq, 1, 1, 1).expand_as(err)
        err = torch.where(keep, err, torch.zeros_like(err))
    bar = BAR * slice_max(ref, n, Lq, heads, dh, nmat, live).clamp(min=1.0)          # [n, nmat, heads]
    ratio = err / bar[:, None, :, :, None]
    bad = ~(ratio <= 1.0)                                                           # (a NaN is bad)
    worst = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    i = int(worst.reshape(-1).argmax())
    s, q, m, h, c = (int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    assert not bool(bad.any()), ('%s: %d values over the per-slice bar; worst at sample %d head %d matrix %d position %d column %d: got %r ref %r '
                                 '(err / bar = %.3g, bar = 2e-5 * %.3g)' % (what, int(bad.sum()), s, h, m, q, c, float(g[s, q, m, h, c]),
                                                                                float(r[s, q, m, h, c]), float(worst[s, q, m, h, c]),
                                                                                float(bar[s, m, h]) / BAR))
    return float(worst.reshape(-1)[i])
