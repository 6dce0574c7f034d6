"""Thin Python wrappers over the C-ABI (one function per entry point of include/nnr_hip.h).
Tensors are only used as (device pointer, size) carriers; views are fine as long as the leading dimension is passed."""
import ctypes as C
import math
import os
import weakref

import torch

from . import _lib as L
from . import profile as _prof
from . import tape as _tape

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
K_CHUNK = 1024      # reduction rows per slice of the token-reduction (weight-gradient) GEMMs, see nnr_gemm_args.k_chunk


class _NoSpan:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NOSPAN = _NoSpan()


def _hbm_span(family, per_row, rows, dyn=None, fixed=0.0, tag=''):
    """Live-profile span of an HBM-bound launch (bench.py `roofline.hbm`): ALGORITHMIC bytes = fixed + per_row x live rows, every
    operand read once and every result written once; `dyn` = device int32 holding the live row count (read after the timed region)."""
    if not _prof.active():
        return _NOSPAN

    def flops(vals=None):
        return 0.0

    def nbytes(vals=None, rows=rows, dyn=dyn):
        r = rows
        if dyn is not None:
            r = min(rows, int(vals[dyn.data_ptr()]) if vals is not None else int(dyn.reshape(-1)[0].item()))
        return float(fixed) + float(per_row) * r
    flops.dyn = [dyn] if dyn is not None else []
    flops.bytes_fn = nbytes
    flops.hbm = True
    flops.tag = tag or 'rows%d%s' % (rows, ' dyn' if dyn is not None else '')
    return _prof.span(family, flops)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise L.NnrHipError('nnr_amd ops need device tensors (no CPU fallback on the product path)')
    return t.data_ptr()


_DEV_INDEX = []


def _s():
    """Raw handle of torch's current HIP stream on this process's device.  (`torch.cuda.current_stream().cuda_stream` costs
    ~9 us of host time per call -- device-index and availability checks --, 170 calls per step; the raw getter ~0.3 us.)"""
    if not _DEV_INDEX:
        _DEV_INDEX.append(torch.cuda.current_device())      # one process per GPU: fixed after set_device
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX[0])


# ---------------------------------------------------------------------------------------------- leaf work on its own stream
# Weight-gradient GEMMs are LEAVES of the backward pass: nothing downstream reads them before the optimizer.  Issued inline
# they sit on the critical chain of the (latency-bound) data-gradient kernels; here they go to a separate HIP stream that
# waits for the producer of their inputs, and the caller joins it before its backward returns (every accumulation into a
# parameter gradient is atomic, so concurrent leaves are safe).  The scope holds a reference to every input until the join,
# so a buffer the caller drops early cannot be handed out again under a pending read.  (`Tensor.record_stream` would do the
# same through the caching allocator, but a recorded multi-GB buffer that is freed while the leaf stream is still busy is
# not reusable until its event completes: the allocator then grows with hipMalloc and the step time turned bimodal,
# 14 ms or 50-67 ms per step -- measured when the 2.7 GB gate buffer was recorded.)
_LEAF = {}
SIDE_CALL = True            # model.Model.forward: candidate encoder call on a side stream (tests switch it off)
EXTRA_STREAMS = []          # every HIP stream this package created (side, title, leaf): see join_extra_streams()


ONE_STREAM = [os.environ.get('NNR_ONE_STREAM') == '1']      # diagnostic: every launch on the caller's stream (solo kernel durations)
STREAM_CACHES = []                                           # dicts of streams handed out by new_stream (dropped when the mode flips)


def set_one_stream(flag):
    """Serialise (True) / restore (False) the package's HIP streams: in serialised mode every launch goes to the caller's stream, so
    the HIP-event spans of nnr_amd.profile are SOLO kernel durations (bench.py's `roofline.isolated`)."""
    torch.cuda.synchronize()
    ONE_STREAM[0] = bool(flag)
    for c in STREAM_CACHES:
        c.clear()
    del EXTRA_STREAMS[:]


def new_stream(dev):
    """A new HIP stream of the package (one per role: side, title, leaf, ...).  (Measured and rejected: a high HIP stream priority for
    the streams that carry a piece of the dependent chain -- 13.43 vs 13.05 ms/step, later no difference.)"""
    if ONE_STREAM[0]:
        return torch.cuda.current_stream(dev)
    # HIP binds a stream to one of its 4 hardware queues (GPU_MAX_HW_QUEUES; 5 and up fall off a cliff: 13 ms per batch-64 step, 6.5 per batch-8 step) and
    # the step runs on 5-6 streams, so some share a queue; WHICH ones do depends on the order the process created and first used its streams, and it
    # decides up to 7 % of the latency-bound batch-8 step: 3.10-3.20 ms in the natural order of a fresh process, 3.3-4.1 ms with 1-4 idle streams in front
    # of the set or of one of its streams; at batch 64 every pattern tried is within 0.08 ms of the natural one (profiles/r06_ab.txt calls 42-46).
    st = torch.cuda.Stream(device=dev)
    EXTRA_STREAMS.append(st)
    return st


STREAM_CACHES.append(_LEAF)
_LEAF_ALT = {}
STREAM_CACHES.append(_LEAF_ALT)


def leaf_stream(dev, alt=False):
    """The leaf stream of `dev` (alt: the second one, see leaf_scope), created on first use."""
    table = _LEAF_ALT if alt else _LEAF
    key = (dev.type, dev.index)
    if key not in table:
        table[key] = new_stream(dev)
    return table[key]


def join_extra_streams(dev=None):
    """Make the current stream wait for everything enqueued on the package's own streams.  Every backward function joins
    the streams it used before it returns; the trainer calls this once more before the gradient exchange / optimizer
    (parameter gradients are written out of autograd's sight, so autograd's own stream bookkeeping does not cover them)."""
    cur = torch.cuda.current_stream(dev)
    for st in EXTRA_STREAMS:
        cur.wait_stream(st)
    _DEFER['keep'].clear()               # leaf_deferred: everything it issued is ordered before the caller's next launch now
    _DEFER['queued'] = False             # (also the recovery path if a backward pass died before its end-of-pass callback ran)


def join_leaf_streams(dev=None):
    """Make the current stream wait for the leaf streams only (weight-gradient launches issued so far), leaving the side / title
    streams alone.  The tensors those launches read stay held until the step's final join_extra_streams()."""
    if dev is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    cur = torch.cuda.current_stream(dev)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    for table in (_LEAF, _LEAF_ALT):
        st = table.get(key)
        if st is not None and st is not cur:
            cur.wait_stream(st)


class leaf_scope:
    """with leaf_scope(device) as leaf:  leaf(fn, *input_tensors)  ...   -- joined on exit.
    defer_join: do NOT make the caller's stream wait for the leaf stream on exit; the leaf work (weight gradients nothing downstream
    reads) is joined by the step's final join_extra_streams(), and the input tensors are held until then.  (Round 4: the user
    encoder's backward ended with the main stream waiting ~150 us for its last weight-gradient GEMMs before the news encoder's
    backward could start -- a dependency only the data-parallel early bucket needs.)"""

    def __init__(self, dev, enable=True, defer_join=False):
        self.dev, self.enable, self.defer_join = dev, enable, defer_join

    def __enter__(self):
        self.keep = []
        if self.enable:
            self.leaf = leaf_stream(self.dev)
            self.leaf2 = None
            self.main = torch.cuda.current_stream(self.dev)
        return self

    def __call__(self, fn, *tensors, alt=False):
        """alt: the SECOND leaf stream (LEAF2, round 4): leaf work of the title token stream, so that it does not queue behind the
        content stream's on small, latency-bound steps."""
        if not self.enable:
            fn()
            return
        st = self.leaf
        if alt and not ONE_STREAM[0]:
            if self.leaf2 is None:
                self.leaf2 = leaf_stream(self.dev, alt=True)
            st = self.leaf2
        st.wait_stream(torch.cuda.current_stream(self.dev))     # the producer of the inputs (may be a side stream)
        self.keep.extend(tensors)
        with torch.cuda.stream(st):
            fn()

    def sync(self):
        """Make the CURRENT stream wait for the leaf work issued so far (for a consumer in the middle of the scope)."""
        if self.enable:
            cur = torch.cuda.current_stream(self.dev)
            cur.wait_stream(self.leaf)
            if self.leaf2 is not None:
                cur.wait_stream(self.leaf2)

    def __exit__(self, *a):
        if self.enable and self.defer_join and a[0] is None:
            _DEFER['keep'].extend(self.keep)      # held until join_extra_streams(): the leaf stream may still be reading them
        elif self.enable:
            self.main.wait_stream(self.leaf)
            if self.leaf2 is not None:
                self.main.wait_stream(self.leaf2)
        self.keep = []                   # (dropped on the host after the join was ENQUEUED: later main-stream work is ordered behind it)


_DEFER = {'keep': [], 'queued': False, 'calls': 0}     # calls: launches that went to the leaf stream (tests)


LEAF_MIN_ROWS = 49152       # defer only when the step is big enough to be GPU-bound (Model.forward posts the history call's token
STEP_ROWS = [0]             # rows here) or the reduction itself is this long: on small, launch-latency-bound steps the cross-stream
                            # dependencies cost more than the overlap gains (CNN+ATT at batch 16: 6 607 impressions/s inline vs
                            # 5 156 deferred; MHSA+MHSA at batch 64: 10 596 inline vs 11 120 with every weight gradient deferred)


def leaf_deferred(dev, rows, fn, *tensors, force=False):
    """Inside an autograd backward function: run `fn` (a weight-gradient launch, atomic accumulation) on the leaf stream
    behind the current stream's work, and join it when THIS backward pass ends (autograd's end-of-pass callback), so the data
    gradient chain on the main stream does not wait for it.  `tensors` (the inputs fn reads) are held until that join.
    _DEFER['off'] (tests) runs fn inline.  force: always on the leaf stream -- for an accumulation that is NOT atomic (bag_mean_bwd: one
    plain writer per table row), whose launches from backward nodes on different streams (the candidate call's on the side stream)
    must not overlap: on the one leaf stream they run one after the other."""
    if not force and (_DEFER.get('off') or max(rows, STEP_ROWS[0]) < LEAF_MIN_ROWS):
        fn()
        return
    leaf, main = leaf_stream(dev), torch.cuda.current_stream(dev)
    if force and leaf == main:           # (one-stream mode: nothing to serialise; the unforced path is as it always was)
        fn()
        return
    leaf.wait_stream(main)
    _DEFER['keep'].extend(tensors)
    _DEFER['calls'] += 1
    with torch.cuda.stream(leaf):
        fn()
    if _DEFER.get('manual'):
        return                           # the native step (nnr_amd.step) joins the leaf stream itself when its backward sequence ends
    if not _DEFER['queued']:
        _DEFER['queued'] = True
        try:                             # end-of-pass callbacks run on the stream that surrounded the caller's backward()
            torch.autograd.Variable._execution_engine.queue_callback(lambda: join_extra_streams(dev))
        except RuntimeError:             # not inside a backward pass (a backward function called by hand): join right away
            join_extra_streams(dev)


def tape_keep(*tensors):
    """A launch tape that is recording right now (nnr_amd.tape) takes a reference to `tensors`: cached device buffers that live in
    module-level tables (W^T copies and their descriptor table, slot / exchange workspaces, packed-gradient accumulators) are replaced
    when a table is rebuilt -- e.g. after other models of the process were garbage-collected -- and a tape must not be left pointing
    at freed memory.  No-op when nothing records."""
    t = _tape.ACTIVE[0]
    if t is not None:
        t.keep.extend(x for x in tensors if x is not None)


# ---------------------------------------------------------------------------------------------- derived weights
# W^T copies (wt), bf16x3 images (bx3_images) and packed LSTM layouts (lstm_pack): buffers computed from the parameters, in one cache.
#   identity   entry key (kind, source); the source is held by weak reference and a tensor source's pointer is checked on every lookup (the
#              caching allocator hands a freed tensor's address to the next tensor of that size -- found with bf16x3 on: 10 GPU tests
#              multiplied by the previous test's weights).  The buffers keep their addresses while the source lives: refreshes refill them.
#   freshness  refreshed when the stamp moved: PARAM_EPOCH (every optimizer step that writes the parameters through raw pointers), the tape
#              that records (a recorded step must hold the refresh of every derived buffer it reads, or its replays would run on the
#              parameters of the recording step), and per source its (pointer, version counter) or, for a derived source, that entry's
#              generation (bumped by every refresh: the images of a W^T copy follow the copy however the parameter changed).
#   streams    a refresh runs on the stream of the first user, or on the leaf stream in a prefetch, and records an event that users on other
#              streams wait for (without it the history call read images the candidate call was still writing: 7.7e-2 gradient error in the
#              two-ranks-on-one-GPU test).  Refilling in place is safe: the last step's readers joined the main stream before the optimizer.
PARAM_EPOCH = [0]
_DERIVED = {}               # (kind, id(source)) -> _Derived
_OWNED = {}                 # id(derived buffer) -> its entry (which holds the buffer: the id cannot be reused while it is listed)
_DERIVED_SWEEP = 256        # a new entry beyond this many first drops every entry whose source has died
_WT_DESCS = [None, None]    # (descriptors, device-resident nnr_transpose_batch table) of the last W^T prefetch


class _Derived:
    __slots__ = ('ref', 'ptr', 'spec', 'out', 'bufs', 'prefetch', 'stamp', 'gen', 'event', 'stream', 'served')


def is_weight(t):
    """A parameter or a buffer of the derived-weight cache: rewritten only when the parameters change, so its bf16x3 images can be cached
    (an activation buffer is rewritten through the C-ABI without any version bump)."""
    return isinstance(t, torch.nn.Parameter) or id(t) in _OWNED


def _drop(key):
    for b in _DERIVED.pop(key).bufs:
        _OWNED.pop(id(b), None)


def _derived(kind, src, spec, make, prefetch):
    """The entry of (kind, src) with layout `spec`; a new one (make(): a tensor, or an object listing its tensors in `bufs`) when there is none
    or it was made for another object, address or layout.  prefetch: the entry may be refreshed by its kind's prefetch at the start of a step."""
    key = (kind, id(src))
    ptr = src.data_ptr() if torch.is_tensor(src) else None
    e = _DERIVED.get(key)
    if e is not None and e.ref() is src and e.ptr == ptr and e.spec == spec:
        return e
    if e is not None:
        _drop(key)
    if len(_DERIVED) > _DERIVED_SWEEP:
        for k in [k for k, v in _DERIVED.items() if v.ref() is None]:
            _drop(k)
    e = _DERIVED[key] = _Derived()
    e.ref, e.ptr, e.spec, e.prefetch = weakref.ref(src), ptr, spec, prefetch
    e.out = make()
    e.bufs = (e.out,) if torch.is_tensor(e.out) else e.out.bufs
    e.stamp, e.gen, e.event, e.stream, e.served = None, 0, None, None, False
    for b in e.bufs:
        _OWNED[id(b)] = e
    return e


def _stamp(sources):
    t = _tape.ACTIVE[0]
    s = [PARAM_EPOCH[0], None if t is None else weakref.ref(t)]
    for x in sources:
        o = _OWNED.get(id(x))
        s.append(o.gen if o is not None else (x.data_ptr(), x._version))
    return tuple(s)


def _refreshed(jobs, stream):
    """jobs = [(entry, stamp)] were just refilled on the current stream (raw handle `stream`): one event for all of them."""
    ev = torch.cuda.Event()
    ev.record()
    for e, stamp in jobs:
        e.stamp, e.gen, e.event, e.stream = stamp, e.gen + 1, ev, stream


def _serve(e, sources, fill):
    """Hand out entry `e` (computed from `sources`) to a launch on the current stream: refilled here by fill() when stale, else ordered behind
    its last refresh."""
    e.served = True
    tape_keep(*e.bufs)
    stamp, cur = _stamp(sources), _s()
    if e.stamp != stamp:
        fill()
        _refreshed([(e, stamp)], cur)
    elif e.stream != cur:
        torch.cuda.current_stream(e.bufs[0].device).wait_event(e.event)


def _stale(kind):
    """[(entry, source, stamp)] of the prefetchable entries of `kind` that were served since the last prefetch (not another model's) and are
    stale."""
    jobs = []
    for (k, _), e in _DERIVED.items():
        src = e.ref() if k == kind and e.prefetch and e.served else None
        if src is not None and src.data_ptr() == e.ptr:
            stamp = _stamp((src,))
            if e.stamp != stamp:
                jobs.append((e, src, stamp))
    return jobs


def _on_leaf(dev, jobs, launch):
    """launch() -- the refresh of jobs = [(entry, source(s), stamp)] -- on the leaf stream, behind the current stream's work (the optimizer step
    that changed the parameters), with one event for all of them."""
    leaf = leaf_stream(dev)
    leaf.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(leaf):
        launch()
        _refreshed([(e, stamp) for e, _, stamp in jobs], _s())
    for e, _, _ in jobs:
        e.served = False


def wt(w):
    """W^T (contiguous [cols, rows]) of a 2-D contiguous weight.  With it every data-gradient GEMM dX = dY . W becomes an NT product (both
    operands K-contiguous) and runs on the LDS-DMA staged kernels; the transposes are a few hundred KB per step against GBs of activations.
    In training, Model.forward / the native step refresh the stale copies of every parameter in one launch on the leaf stream (wt_prefetch),
    so the backward pass only ever finds fresh ones."""
    rows, cols = w.shape
    e = _derived('wt', w, (rows, cols), lambda: torch.empty((cols, rows), device=w.device, dtype=torch.float32), isinstance(w, torch.nn.Parameter))
    _serve(e, (w,), lambda: transpose2d(w, e.out, rows, cols))
    return e.out


def wt_prefetch(dev):
    """Refresh, on the leaf stream and in ONE launch (nnr_transpose_batch over a device-resident descriptor table), the stale W^T copies of the
    parameters wt() served since the last prefetch (i.e. after an optimizer step).  Called at the start of a training forward pass: the copies
    are needed by the BACKWARD pass only, so they leave the critical chain -- made lazily, the first user's stream does the copy and users on
    the other streams wait for it (measured: a 383 us stall of the history call's backward behind the candidate call's)."""
    if torch.cuda.is_current_stream_capturing():        # (under hipGraph capture the copies are refreshed lazily by wt(): ending a
        return                                          # capture that holds this fork segfaults in the HIP runtime)
    jobs = _stale('wt')
    if not jobs:
        return
    descs = tuple((w.data_ptr(), e.out.data_ptr(), w.shape[0], w.shape[1]) for e, w, _ in jobs)
    if _WT_DESCS[0] != descs:
        arr = (L.TransposeDesc * len(descs))()
        for d, (src, out, rows, cols) in zip(arr, descs):
            d.inp, d.out, d.rows, d.cols = src, out, rows, cols
        _WT_DESCS[:] = [descs, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)]
    table = _WT_DESCS[1]
    tape_keep(table, *[e.out for e, _, _ in jobs])
    _on_leaf(dev, jobs, lambda: L.check(L.lib().nnr_transpose_batch(_p(table), len(descs), _s()), 'nnr_transpose_batch'))


def _pack_entry(lstm, p, H, E):
    return _derived('lstm', lstm, (H, E), lambda: LstmPacked(p, H, E, fill=False), False)


def lstm_pack(lstm, H, E):
    """The parameters of `lstm` (layers.LSTMParams) in the recurrent kernels' layouts (LstmPacked), refilled in place when they changed (once
    per optimizer step: both encoder calls of a step share them)."""
    p = lstm.param_list()
    e = _pack_entry(lstm, p, H, E)
    _serve(e, p, lambda: e.out.pack(p))
    return e.out


def lstm_prefetch(dev, lstms, H, E):
    """Refresh the stale packs of `lstms` on the leaf stream, one event for all: they need nothing of the step but the parameters, so they run
    next to the planner / row gather of the chains; each chain waits for them in front of its input projection (lstm_pack)."""
    jobs = []
    for lstm in lstms:
        p = lstm.param_list()
        e = _pack_entry(lstm, p, H, E)
        stamp = _stamp(p)
        if e.stamp != stamp:
            jobs.append((e, p, stamp))

    def launch():
        for e, p, _ in jobs:
            tape_keep(*e.bufs)
            e.out.pack(p)
    if jobs:
        _on_leaf(dev, jobs, launch)


def _tn_sized(tile, target):
    t = L.gemm_tiles()[tile or 2]        # (0: the library chooses; its register-staged fallback for TN is the 64 x 80 tile 2)
    return tile, t.rows, t.cols, target


def tn_tile(M, N, K, gather=False):
    """Tile of a token-reduction (weight-gradient) GEMM C[M,N] += A[K,M]^T B[K,N] and the tile dims its split-K factor is sized
    for: the LDS-DMA staged tiles of csrc/gemm.hip (gemm_tn_pipe_kernel) as (tile id, rows, cols, workgroups to aim for).  Measured
    on the step's shapes (tools/gemm_pipe_bench.py tn, TFLOP/s old -> new): 1664x300 82 -> 96 (128x80), 832x200 with gathered rows
    68 -> 86, 400x400 75 -> 82, 200x400 62 -> 73 (128x208); short reductions stay on the register-staged 64x80 tile.  (The 53 KB
    128 x 80 tile everywhere lost to the 78 KB 128 x 208 one for N = 200 / 400 once the recurrence held 120-130 KB: 11.43 vs 11.38 ms.)"""
    if K >= 2048 and M >= 512 and N >= 512 and not gather and not ((M & 3) or (N & 3)):
        return _tn_sized(26, 2048)            # SUE's 900 x 900 x 4 352 weight gradients: 8 slices of 544 rows instead of 12 of 363 on the 64 x 80 tile
    if K < 8192 or (M & 3) or (N & 3) or (M >= 512 and N >= 512):
        return _tn_sized(0, 2048)
    if not gather and M >= 1024 and 160 < N <= 320:
        return _tn_sized(30, 2048)            # 128 x 160: dW_ih (1664 x 300): operand counter traffic 2.0x -> 1.5x -- A (d gates) is fetched twice, not 4x
    if N <= 208 or (N > 320 and N <= 416):
        if gather or M % 128 != 0:
            return _tn_sized(32, 640)         # gen-2 loop, 64 x 208: M = 200 / 400 / 832 in 4 / 7 / 13 row tiles (256 / 448 / 832 rows of MFMA work, not 256 / 512 / 896)
        return _tn_sized(27, 640)             # gen-2 loop, 128 x 208 (one token row per DMA instruction: takes gathered rows)
    if gather:
        return _tn_sized(20, 2048)            # 128 x 80: gathered rows wider than 208 columns (dW_hh at --hidden_dim 212..256): tile 26 has no gather path
    return _tn_sized(26, 2048)                # gen-2 loop, 128 x 80


def split_for(m, n, k, tile_m=64, tile_n=80, target_blocks=2048, kmin=256):
    """split-K factor for the token-reduction (weight-gradient) GEMMs: enough blocks to fill 256 CUs x ~3.  (Cutting short
    reductions finer, kmin 64, measured no better.)"""
    tiles = max(1, ((m + tile_m - 1) // tile_m) * ((n + tile_n - 1) // tile_n))
    if k <= 640:
        return 1      # a few hundred reduction rows (the per-candidate projections: 320 rows at batch 64): one slice -- no slab, no second launch
    return int(max(1, min((k + kmin - 1) // kmin, (target_blocks + tiles - 1) // tiles)))


# ---------------------------------------------------------------------------------------------- bf16x3 NT GEMMs (the default matrix path since round 6)
# The GPU-filling NT launches whose B operand is a weight (a parameter, a cached transpose, the packed LSTM input weights) run on
# csrc/gemm.hip:gemm_nt_bx3_kernel: fp32 arithmetic as six exact bf16 x bf16 products with fp32 accumulation: the same
# fp32 inputs, fp32 outputs, and a third of the fp32-MFMA kernel's error against fp64.  The weight's three bf16 images are derived weights (see
# above): re-split when the weight changed -- one small launch per weight and step, recorded in the launch tape
# like any other call.  Round 5 measured it (off); round 6 made it the default after five interleaved same-box pairs + a per-shape-class A/B
# (profiles/r06_bx3_phases.md: -0.33 ms of the 10.27 ms headline step, every class positive).  NNR_BX3=0 = the pure fp32-MFMA path
# (bench.py keeps it as a `secondary` leg of the same workload so that both numbers are driver-timed).
BX3 = [os.environ.get('NNR_BX3', '1') == '1']
_BX3_MIN_ROWS = 2048
_BX3_TILE = 50          # 128 x 80, 2 workgroups / CU (tile 51, 64 x 80 with 3 per CU, stays for explicit callers)
# shape classes the bf16x3 kernel takes (round 6: decided per class by same-box in-step A/Bs, profiles/r06_bx3_phases.md):
#   dx   = long reductions (K >= 1024: the embedding-row gradient dX = dGates . W_ih, K = 2 NP = 1664)
#   sue  = K >= 800 (the user encoder's 900 x 900 layers)
#   proj = N >= 1024 (the LSTM input projection x . W_ih^T, N = 1664)
#   gate = everything else (gate / attention projections, K, N = 200 .. 400)
_BX3_CLASSES = {'dx', 'sue', 'proj', 'gate'}      # (step.matrix_path narrows it per model and step size)


def bx3_class(N, K):
    if K >= 1024:
        return 'dx'
    if K >= 800:
        return 'sue'
    if N >= 1024:
        return 'proj'
    return 'gate'


BX3_SEEN = {}                                                  # diagnostics: (M, N, K, 'weight' | 'other') -> launches that met every other condition


def _split_bf16x3(B, N, K, ldb, img):
    ldo = img.shape[2]
    L.check(L.lib().nnr_split_bf16x3(_p(B), N, K, ldb, ldo, _p(img), N * ldo, _s()), 'nnr_split_bf16x3')


def bx3_prefetch(dev):
    """Re-split, on the leaf stream at the start of a training step (right behind wt_prefetch's transposes, same stream), the stale bf16 images
    of every parameter and cached transpose bx3_images() served since the last prefetch (i.e. after an optimizer step).  Made lazily, each split
    is a 3-30 us launch on the stream of its first user -- five of them sat on the step's dependent chain in front of their GEMMs
    (profiles/r06_ab.txt: split_bf16x3_kernel 21 / 11 / 34 / 28 / 14 us on the main streams).  The images of the packed LSTM weights, re-packed
    inside the forward pass, are split by their first user."""
    if not BX3[0] or torch.cuda.is_current_stream_capturing():
        return
    jobs = _stale('bx3')

    def launch():
        for e, B, _ in jobs:
            tape_keep(e.out, B)                   # (B: a parameter -- inside the trainer's flat buffer -- or a long-lived cached transpose)
            _split_bf16x3(B, *e.spec, e.out)
    if jobs:
        _on_leaf(dev, jobs, launch)


def bx3_images(B, N, K, ldb):
    """(images [3, N, ldo] bf16-as-int16, image stride in elements, ldo) of the [N, K] weight `B` (a derived-weight-cache entry: re-split when
    `B` changed)."""
    ldo = (K + 7) // 8 * 8
    owner = _OWNED.get(id(B))
    e = _derived('bx3', B, (N, K, ldb), lambda: torch.empty((3, N, ldo), device=B.device, dtype=torch.int16),
                 isinstance(B, torch.nn.Parameter) or (owner is not None and owner.prefetch))
    _serve(e, (B,), lambda: _split_bf16x3(B, N, K, ldb, e.out))
    return e.out, N * ldo, ldo


def _bx3_wanted(A, B, M, N, K, lda, ldb, trans_a, trans_b, a_idx, b_idx, c_idx, split_k, k_chunk, rowdot_w, colsum_out, atomic, batch, dyn_dim, drop):
    return (not trans_a and not trans_b and a_idx is None and b_idx is None and split_k <= 1 and k_chunk <= 0 and rowdot_w is None
            and colsum_out is None and batch <= 1 and dyn_dim in (0, 1) and M >= _BX3_MIN_ROWS and K >= 64 and N * K <= (1 << 22)
            and (K | lda | ldb) & 3 == 0 and (A.data_ptr() | B.data_ptr()) & 15 == 0 and (drop is None or drop[0] in (3, 4) or drop[1] <= 0.0))


def gemm_family(g):
    """The live profile's kernel family of the launch nnr_gemm_f32 makes for the filled argument struct `g`: asked of the library
    (nnr_gemm_tile_for -- the function the launch itself chooses with), named from its tile table."""
    t = L.lib().nnr_gemm_tile_for(C.byref(g))
    L.check(min(t, 0), 'nnr_gemm_f32', counted=False)
    tiles = L.gemm_tiles()
    return 'gemm_%s_%s' % ('tn' if g.trans_a else ('nn' if g.trans_b else 'nt'), tiles[t].suffix if t in tiles else 'tile%d' % t)


def gemm(A, B, C_=None, *, M, N, K, lda, ldb, ldc=0, trans_a=False, trans_b=False, dyn=None, dyn_dim=0, a_idx=None, b_idx=None,
         drop=None, alpha=1.0, bias=None, rowvec=None, ldrv=0, rowvec_map=None, act=0, aux_out=None, ldaux=0, mul=None, ldmul=0,
         resid=None, ldres=0, accumulate=False, atomic=False, c_idx=None, split_k=1, rowdot_w=None, rowdot_out=None, batch=1,
         strideA=0, strideB=0, strideC=0, stride_aux=0, stride_res=0, tile=0, colsum_out=None, k_chunk=0, flop_scale=1.0, slab=None,
         pre_add=None, ldpre=0, gate_bwd=False, b3=None):
    # flop_scale: algorithmic / padded work of this launch (the LSTM gate columns are padded 800 -> 832 per direction; the live
    # profile counts the true 8H columns, not the padded 2*NP)
    # ctypes zero-initialises the struct: only the fields a call actually uses are written (a field store costs ~0.2 us of host
    # time and a step issues ~130 GEMMs; writing all ~50 fields was the largest single item of the host-side enqueue time)
    g = L.GemmArgs()
    g.A, g.B = A.data_ptr(), B.data_ptr()
    if C_ is not None:
        g.C = C_.data_ptr()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.alpha = M, N, K, lda, ldb, ldc, alpha
    if trans_a:
        g.trans_a = 1
    if trans_b:
        g.trans_b = 1
    if dyn is not None:
        g.dyn_dev, g.dyn_dim = dyn.data_ptr(), dyn_dim
    if a_idx is not None:
        g.a_idx = a_idx.data_ptr()
    if b_idx is not None:
        g.b_idx = b_idx.data_ptr()
    if drop is not None and drop[1] > 0.0:
        g.drop_target, g.drop_p, g.drop_seed, g.drop_cols = drop[0], float(drop[1]), int(drop[2]), int(drop[3])
    if bias is not None:
        g.bias = bias.data_ptr()
    if rowvec is not None:
        g.rowvec, g.ldrv, g.rowvec_map = rowvec.data_ptr(), ldrv, _p(rowvec_map)
    if act:
        g.act = act
    if aux_out is not None:
        g.aux_out, g.ldaux = aux_out.data_ptr(), ldaux
    if mul is not None:
        g.mul, g.ldmul = mul.data_ptr(), ldmul
    if resid is not None:
        g.resid, g.ldres = resid.data_ptr(), ldres
    if accumulate:
        g.accumulate = int(accumulate)
    if atomic:
        g.atomic = 1
    if c_idx is not None:
        g.c_idx = c_idx.data_ptr()
    g.split_k, g.batch = int(split_k), batch
    if rowdot_w is not None:
        g.rowdot_w, g.rowdot_out = rowdot_w.data_ptr(), rowdot_out.data_ptr()
    if batch > 1:
        g.strideA, g.strideB, g.strideC, g.stride_aux, g.stride_res = strideA, strideB, strideC, stride_aux, stride_res
    if tile:
        g.tile = tile
    if colsum_out is not None:
        g.colsum_out = colsum_out.data_ptr()
    if k_chunk:
        g.k_chunk = int(k_chunk)
    if pre_add is not None:
        g.pre_add, g.ldpre = pre_add.data_ptr(), ldpre
    if gate_bwd:
        g.gate_bwd = 1
    if b3 is None and BX3[0] and tile in (0, 9, 15, 16) and _bx3_wanted(A, B, M, N, K, lda, ldb, trans_a, trans_b, a_idx, b_idx, c_idx, split_k, k_chunk, rowdot_w,
                                                                    colsum_out, atomic, batch, dyn_dim, drop):
        # (NNR_BX3, default on): this NT launch on the BF16 matrix pipe, weights pre-split.  Only when B IS a weight (is_weight)
        is_w = is_weight(B)
        key = (M, N, K, 'weight' if is_w else 'other')
        BX3_SEEN[key] = BX3_SEEN.get(key, 0) + 1
        if is_w and bx3_class(N, K) in _BX3_CLASSES:
            b3 = bx3_images(B, N, K, ldb)
            tile = _BX3_TILE
            g.tile = _BX3_TILE
    if b3 is not None:
        g.B3, g.b3_stride, g.ldb3 = b3[0].data_ptr(), b3[1], b3[2]
    if slab is None and TN_SLAB and trans_a and trans_b and split_k > 1 and not k_chunk and c_idx is None and (N & 3) == 0 and C_ is not None:
        slab = _slab_ws(A.device, int(split_k) * (M * N + M))      # reproducible split-K: partial results to a slab + fixed-order reduction
    if slab is not None:
        g.slab, g.slab_floats = slab.data_ptr(), slab.numel()
    if not (A.is_cuda and B.is_cuda):
        raise L.NnrHipError('nnr_amd ops need device tensors (no CPU fallback on the product path)')
    if not _prof.active():
        L.check(L.lib().nnr_gemm_f32(C.byref(g), _s()), 'nnr_gemm_f32')
        return
    fam = gemm_family(g)

    def flops(vals=None, M=M, N=N, K=K, dyn=dyn, dyn_dim=dyn_dim, batch=batch):
        # vals: {data_ptr of a device-side size: its value at the time of the launch} (replayed launches: the size buffers are
        # overwritten by the next step, so the trainer snapshots them per timed replay); None: read the buffer now
        m, k = M, K
        if dyn is not None:
            d = int(vals[dyn.data_ptr()]) if vals is not None else int(dyn.item())
            m, k = (min(M, d), K) if dyn_dim == 1 else (M, min(K, d))
        return 2.0 * m * N * k * max(1, batch) * flop_scale
    flops.dyn = [dyn] if dyn is not None else []
    flops.scale = flop_scale                         # algorithmic / executed (padded gate columns): bench.py reports both sums

    def op_bytes(vals=None, M=M, N=N, K=K, dyn=dyn, dyn_dim=dyn_dim, batch=batch):
        # algorithmic HBM bytes of the launch: A and B read once, C written once (+ read when accumulated into), every extra
        # epilogue stream (aux_out, mul, resid) once; true extents
        m, k = M, K
        if dyn is not None:
            d = int(vals[dyn.data_ptr()]) if vals is not None else int(dyn.item())
            m, k = (min(M, d), K) if dyn_dim == 1 else (M, min(K, d))
        outs = (1 if C_ is not None else 0) + (1 if accumulate else 0) + (1 if aux_out is not None else 0) + (1 if mul is not None else 0) + (1 if resid is not None else 0) + (1 if pre_add is not None else 0)
        return 4.0 * max(1, batch) * (m * k + N * k + m * N * outs)
    flops.bytes_fn = op_bytes
    if trans_a and trans_b and split_k > 1:
        flops.tn_dims = (M, N, flop_scale)           # token-reduction GEMM: operand bytes of the launch = live reduction rows x (M + N) x 4
    flops.tag = 'M%d N%d K%d%s%s%s' % (M, N, K, ' b%d' % batch if batch > 1 else '', (' sk%d' % split_k if split_k > 1 else '') + (' kc%d' % k_chunk if k_chunk > 0 else ''), ' dyn' if dyn is not None else '')
    with _prof.span(fam, flops):
        L.check(L.lib().nnr_gemm_f32(C.byref(g), _s()), 'nnr_gemm_f32')


def linear_fwd(x, w, bias=None, out=None, act=0, **kw):
    """out[M,N] = act(x[M,K] . w[N,K]^T + bias) for contiguous 2-D x."""
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    gemm(x, w, out, M=M, N=N, K=K, lda=x.stride(0), ldb=w.stride(0), ldc=out.stride(0), bias=bias, act=act, **kw)
    return out


def linear_bwd_data(dy, w, out=None, accumulate=False, **kw):
    """dx[M,K] (+)= dy[M,N] . w[N,K]"""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty((M, K), device=dy.device, dtype=torch.float32)
    if M >= 1024 and w.is_contiguous() and (N & 3) == 0:
        gemm(dy, wt(w), out, M=M, N=K, K=N, lda=dy.stride(0), ldb=N, ldc=out.stride(0), accumulate=accumulate, **kw)      # NT on W^T
    else:
        gemm(dy, w, out, M=M, N=K, K=N, lda=dy.stride(0), ldb=w.stride(0), ldc=out.stride(0), trans_b=True, accumulate=accumulate, **kw)
    return out


def linear_bwd_weight(dy, x, dw, dyn=None, rows=None, db=None, small_lds=False, **kw):
    """dw[N,K] += dy[rows,N]^T . x[rows,K]   (split-K atomics; dw must already hold the running gradient);
    db[N] += column sums of dy, fused into the same launch.  small_lds: the 19 KB register-staged tile (for launches meant to run
    beside the recurrence, whose workgroups hold 120-130 KB of LDS per CU)."""
    R = dy.shape[0] if rows is None else rows
    N, K = dw.shape
    t, bm, bn, target = tn_tile(N, K, R)
    if small_lds:
        t, bm, bn, target = _tn_sized(2, 2048)
    if t and ((dy.stride(0) | x.stride(0)) & 3 or (dy.data_ptr() | x.data_ptr()) & 15):
        t, bm, bn, target = _tn_sized(0, 2048)
    gemm(dy, x, dw, M=N, N=K, K=R, lda=dy.stride(0), ldb=x.stride(0), ldc=dw.stride(0), trans_a=True, trans_b=True,
         atomic=True, dyn=dyn, dyn_dim=2, colsum_out=db, split_k=split_for(N, K, R, bm, bn, target), tile=t, **kw)


def rowdot(x, w, out, dyn=None, rows=None):
    """out[row] = <x[row], w> for the live rows of a 2-D x (the w2 . tanh(.) attention score)."""
    R = x.shape[0] if rows is None else rows
    L.check(L.lib().nnr_rowdot(_p(x), x.stride(0), _p(w), _p(dyn), R, x.shape[1], _p(out), _s()), 'nnr_rowdot')


_SLOT_WS = {}
_SLAB_WS = {}
TN_SLAB = True      # split-K weight gradients through slabs + a fixed-order reduction (False, tests: f32 atomics)
# fixed-order stream-K for the one-to-two-wave NT launches of the user encoder (csrc/gemm.hip: gemm_nt_sk_kernel; round 5, verdict item 1b)
def _slab_ws(dev, floats):
    """Split-K slab workspace of the CURRENT stream (nnr_gemm_args.slab): a launch's slices store their partial results there and the
    reduction that follows it on the same stream consumes them, so launches of one stream share one buffer (grown when a bigger
    launch comes along; a recording tape keeps every buffer it has seen alive)."""
    key = torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    ws = _SLAB_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = torch.empty(max(int(floats), 1 << 22), device=dev, dtype=torch.float32)
        _SLAB_WS[key] = ws
    tape_keep(ws)
    return ws



def _slot_ws(dev, n):
    """Slot workspace of the CURRENT stream (see nnr_slot_workspace_floats): kernels of one stream run in order and each call
    overwrites the slot rows it reads, so one buffer per stream serves every call; grown when a wider vector comes along."""
    key = torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    need = L.lib().nnr_slot_workspace_floats(n)
    ws = _SLOT_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(max(need, 32 * 1024), device=dev, dtype=torch.float32)
        _SLOT_WS[key] = ws
    tape_keep(ws)
    return ws


def bias_grad(dy, db, dyn=None, rows=None):
    R = dy.shape[0] if rows is None else rows
    ws = _slot_ws(dy.device, db.numel())         # per-workgroup slot rows + fixed-order reduction (reproducible; round 3: only for R >= 1024)
    L.check(L.lib().nnr_colsum(_p(dy), dy.stride(0), _p(dyn), R, db.numel(), _p(db), _p(ws), _s()), 'nnr_colsum')


# ---------------------------------------------------------------------------------------------- planner / LSTM
class SeqPlan:
    """Device-resident plan of one token stream (see csrc/seq_plan.hip).  With mask1 / ids1 given the stream is the UNION of two
    encoder calls: sequences [0, n0) from (mask, ids), [n0, n0 + n1) from (mask1, ids1)."""

    def __init__(self, mask, ids, perm=None, mask1=None, ids1=None):
        n0, Lx = mask.shape
        n = n0 + (mask1.shape[0] if mask1 is not None else 0)
        dev = mask.device
        self.n, self.L, self.n0 = n, Lx, n0
        i32 = dict(device=dev, dtype=torch.int32)
        self.len = torch.empty(n, **i32)
        self.order = torch.empty(n, **i32)
        self.rank = torch.empty(n, **i32)
        self.slen = torch.empty(n, **i32)
        self.bs = torch.empty(Lx, **i32)
        self.off = torch.empty(Lx + 1, **i32)
        self.row_seq = torch.empty(n * Lx, **i32)
        self.tok = torch.empty(n * Lx, **i32) if ids is not None else None
        self.prev_f = torch.empty(n * Lx, **i32)
        self.prev_r = torch.empty(n * Lx, **i32)
        self.total = self.off[Lx:]                 # device int32 view: number of valid tokens
        self.cap = n * Lx
        m8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        assert m8.is_contiguous() and (ids is None or (ids.is_contiguous() and ids.dtype == torch.int32))
        outs = (_p(self.len), _p(self.order), _p(self.rank), _p(self.slen), _p(self.bs), _p(self.off), _p(self.row_seq), _p(self.tok),
                _p(self.prev_f), _p(self.prev_r), _s())
        if mask1 is None:
            L.check(L.lib().nnr_seq_plan(_p(m8), _p(ids), n, Lx, _p(perm), *outs), 'nnr_seq_plan')
        else:
            m81 = mask1.view(torch.uint8) if mask1.dtype == torch.bool else mask1
            assert m81.is_contiguous() and m81.shape[1] == Lx and (ids is None) == (ids1 is None)
            assert ids1 is None or (ids1.is_contiguous() and ids1.dtype == torch.int32)
            L.check(L.lib().nnr_seq_plan_pair(_p(m8), _p(ids), n0, _p(m81), _p(ids1), n - n0, Lx, _p(perm), *outs), 'nnr_seq_plan_pair')


def cne_pair_map(plan_t, plan_c):
    """(pm_t, pm_c): per-call rank pairing of two union plans (csrc/seq_plan.hip, section D)."""
    n, n0 = plan_t.n, plan_t.n0
    assert plan_c.n == n and plan_c.n0 == n0
    buf = torch.empty(6 * n, device=plan_t.order.device, dtype=torch.int32)
    pm_t, pm_c = buf[:n], buf[n:2 * n]
    L.check(L.lib().nnr_cne_pair_map(_p(plan_t.order), _p(plan_c.order), n0, n, _p(pm_t), _p(pm_c), _p(buf[2 * n:]), _s()), 'nnr_cne_pair_map')
    return pm_t, pm_c


def lstm_dims(H):
    ub, hp, np_ = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().nnr_lstm_dims(H, C.byref(ub), C.byref(hp), C.byref(np_)), 'nnr_lstm_dims(H=%d)' % H)
    return ub.value, hp.value, np_.value


class LstmPacked:
    """nn.LSTM parameters `p` (in nn.LSTM order) re-laid out for the recurrent kernels (csrc/lstm.hip); pack(p) refills the buffers in place
    (fill=False: allocate only)."""

    def __init__(self, p, H, E, fill=True):
        ub, hp, np_ = lstm_dims(H)
        f = dict(device=p[0].device, dtype=torch.float32)
        self.UB, self.HP, self.NP, self.H, self.E = ub, hp, np_, H, E
        self.w_ihp = torch.empty((2 * np_, E), **f)
        self.b_p = torch.empty(2 * np_, **f)
        self.wf = torch.empty(2 * ub * 4 * ub * 256, **f)
        self.wb = torch.empty(2 * ub * (np_ // 16) * 256, **f)
        self.w_ihp_t = torch.empty((E, 2 * np_), **f)             # [E, 2*NP]: K-contiguous B operand of the dX GEMM (NT form)
        self.bufs = (self.w_ihp, self.b_p, self.wf, self.wb, self.w_ihp_t)
        if fill:
            self.pack(p)

    def pack(self, p):
        L.check(L.lib().nnr_lstm_pack_weights(*[_p(t) for t in p], self.H, self.E, _p(self.w_ihp), _p(self.b_p), _p(self.wf), _p(self.wb),
                                              _p(self.w_ihp_t), _s()), 'nnr_lstm_pack_weights')


def lstm_unpack_grads(dw_ihp, db_p, dw_hhp, H, E, grads, zero_src=False):
    """grads: 8 tensors in nn.LSTM order (w_ih, w_hh, b_ih, b_hh, then *_reverse); accumulated into with f32 atomics
    (parameter gradients may be accumulated from several HIP streams at once).  zero_src: leave the packed buffers zeroed."""
    L.check(L.lib().nnr_lstm_unpack_grads(_p(dw_ihp), _p(db_p), _p(dw_hhp), H, E, *[_p(t) for t in grads], 1, zero_src, _s()),
                                          'nnr_lstm_unpack_grads')


# 2-CU weights-stationary recurrence (lstm.hip).  The library takes it for every even H in 194 .. 208 (13 unit blocks) when each problem of a
# launch carries a `sync` workspace (include/nnr_hip.h); this module hands workspaces out at the product's H = 200 only and passes a caller's
# own `sync` through untouched at any other H.
LSTM_PAIR = os.environ.get('NNR_LSTM_PAIR', '1') != '0'
LAST_LSTM_SYNC = []                                           # exchange workspaces of the last launch (diagnostics)
_TMO = {}                                                     # per device: persistent exchange time-out counter (uint32 as int32)


def _timeout_counter(dev):
    """The device counter every pair-kernel launch of this process adds its exchange time-outs to (registered once with the
    library: nnr_lstm_set_timeout_counter).  One process drives one GPU."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _TMO.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=dev)
        _TMO[key] = t
        L.check(L.lib().nnr_lstm_set_timeout_counter(t.data_ptr()), 'nnr_lstm_set_timeout_counter')
    return t


def dp_busy(buf, workgroups, iters):
    """Diagnostics: `workgroups` resident 512-thread workgroups sweeping `buf` on the CURRENT stream (a stand-in for RCCL's ring kernels)."""
    L.check(L.lib().nnr_dp_busy(_p(buf), buf.numel(), workgroups, iters, _s()), 'nnr_dp_busy')


def lstm_sync_timeouts(reset=False):
    """Exchange time-outs of the CU-pair recurrence accumulated over EVERY launch since the process started (or since the
    last reset); must be 0.  A time-out poisons the step with NaN (the optimizer then skips it).  Synchronises."""
    n = sum(int(t.item()) for t in _TMO.values())
    if reset:
        for t in _TMO.values():
            t.zero_()
    return n


def lstm_last_launch_timeouts():
    """Time-outs recorded by the LAST pair-kernel launch only, read from the diagnostics block of its workspaces at the offset
    the library reports (nnr_lstm_sync_diag_offset).  Synchronises."""
    return sum(int(t[off // 4].item()) for t, off in LAST_LSTM_SYNC)


_SYNC_WS = {}


def _sync_workspace(dev, n, slot):
    """Exchange workspace of the CU-pair recurrence: zero-filled once, then reused launch after launch (the words carry a launch
    epoch, csrc/lstm.hip).  One per (stream kind, direction of the pass, HIP stream): launches that can be in flight together never share one."""
    key = (dev.index, n, slot, torch._C._cuda_getCurrentRawStream(_DEV_INDEX[0] if _DEV_INDEX else torch.cuda.current_device()))      # (per launch stream)
    ws = _SYNC_WS.get(key)
    if ws is None:
        ws = _SYNC_WS[key] = torch.zeros(L.lib().nnr_lstm_sync_bytes(n) // 4, dtype=torch.int32, device=dev)
    tape_keep(ws)
    return ws


def _lstm_probs(items, H=0, backward=False):
    arr = (L.LstmProblem * len(items))()
    del LAST_LSTM_SYNC[:]
    for a, it in zip(arr, items):
        pl = it['plan']
        if LSTM_PAIR and H == 200:
            _timeout_counter(it['gates'].device)
            it['sync'] = _sync_workspace(it['gates'].device, pl.n, (it.get('name'), len(LAST_LSTM_SYNC), backward))
            LAST_LSTM_SYNC.append((it['sync'], L.lib().nnr_lstm_sync_diag_offset(pl.n)))
        a.sync = _p(it.get('sync'))
        a.bs, a.off, a.slen, a.prev_f, a.prev_r = _p(pl.bs), _p(pl.off), _p(pl.slen), _p(pl.prev_f), _p(pl.prev_r)
        a.n, a.L = pl.n, pl.L
        a.gates, a.cell, a.hout, a.cn = _p(it['gates']), _p(it['cell']), _p(it.get('hout')), _p(it.get('cn'))
        a.wf, a.wb = _p(it['w'].wf), _p(it['w'].wb)
        a.dh, a.dcn = _p(it.get('dh')), _p(it.get('dcn'))
    return arr


def _lstm_flops(items, H):
    totals = [it['plan'].total for it in items]

    def flops(vals=None):
        tok = sum(float(vals[t.data_ptr()]) if vals is not None else float(t.item()) for t in totals)
        return tok * 2 * (2.0 * H * 4 * H)                                          # tokens x 2 directions x [1,H]x[H,4H]
    flops.dyn = totals
    flops.scale = 4.0 * H / max(4 * H, -(-H // 16) * 64, 1)   # (H = 0: the entry point refuses the size, not this division)  the kernels multiply NP = ceil(H / 16) x 64 gate columns per direction (H = 200: 832 for 800)
    return flops


def lstm_fwd(items, H):
    arr = _lstm_probs(items, H)
    with _prof.span('lstm_fwd', _lstm_flops(items, H)):
        L.check(L.lib().nnr_lstm_fwd(arr, len(items), H, _s()), 'nnr_lstm_fwd')


def lstm_bwd(items, H):
    arr = _lstm_probs(items, H, backward=True)
    with _prof.span('lstm_bwd', _lstm_flops(items, H)):
        L.check(L.lib().nnr_lstm_bwd(arr, len(items), H, _s()), 'nnr_lstm_bwd')


# ---------------------------------------------------------------------------------------------- GRU
GRU_UNSUPPORTED = 'unsupported size (hidden_dim must be in 1 .. 256 and max_history_num in 1 .. 255)'


def gru_supported(H, T):
    """Host mirror of nnr_gru_dims' rule (csrc/gru.hip), for the constructors: no library call, no device."""
    return 1 <= int(H) <= 256 and 1 <= int(T) <= 255


def gru_dims(H, T=1):
    """(UB, HP, NP) of hidden size H: unit blocks, padded units, padded slot columns (four per unit)."""
    ub, hp, np_ = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().nnr_gru_dims(H, T, C.byref(ub), C.byref(hp), C.byref(np_)), 'nnr_gru_dims(H=%d, T=%d)' % (H, T), GRU_UNSUPPORTED, counted=False)
    return ub.value, hp.value, np_.value


def gru_pack_host(w_ih, w_hh, b_ih, b_hh):
    """Host mirror of nnr_gru_pack_weights on CPU tensors: (w_ihp [NP, D], b_p [NP], wf, wb), element for element what the kernel writes."""
    H, D = w_hh.shape[1], w_ih.shape[1]
    UB = (H + 15) // 16
    NP, HP = UB * 64, UB * 16
    unit = torch.arange(HP)
    live = unit < H
    u = unit.clamp(max=H - 1)
    w_ihp = torch.zeros((UB, 16, 4, D), dtype=w_ih.dtype)
    b_p = torch.zeros((UB, 16, 4), dtype=w_ih.dtype)
    whh_p = torch.zeros((UB, 16, 4, HP), dtype=w_ih.dtype)              # W_hh rows in p-order (slot 2 zero), columns padded
    for slot, gx, gh in ((0, 0, 0), (1, 1, 1), (2, 2, None), (3, None, 2)):
        if gx is not None:
            w_ihp[:, :, slot] = (w_ih[gx * H + u] * live[:, None]).view(UB, 16, D)
        if gh is not None:
            whh_p[:, :, slot, :H] = (w_hh[gh * H + u] * live[:, None]).view(UB, 16, H)
        bias = (b_ih[gx * H + u] if gx is not None else 0) + (b_hh[gh * H + u] if gh is not None else 0)
        b_p[:, :, slot] = (bias * live).view(UB, 16)
    # wf[ub][g][kg][lane][ii] = w_hh[g*H + ub*16 + (lane & 15)][16 kg + 4 (lane >> 4) + ii]
    whh = torch.zeros((3, HP, HP), dtype=w_ih.dtype)
    whh[:, :H, :H] = w_hh.view(3, H, H)
    wf = whh.view(3, UB, 16, UB, 4, 4).permute(1, 0, 3, 4, 2, 5).contiguous().view(-1)        # [ub][g][kg][lane >> 4][lane & 15][ii]
    # wb[ubn][kg][lane][ii] = whh_p[p = 16 kg + 4 (lane >> 4) + ii][ubn*16 + (lane & 15)]
    wb = whh_p.view(NP // 16, 4, 4, UB, 16).permute(3, 0, 1, 4, 2).contiguous().view(-1)      # [ubn][kg][lane >> 4][lane & 15][ii]
    return w_ihp.view(NP, D), b_p.view(NP), wf, wb


class GruPacked:
    """nn.GRU parameters `p` = (w_ih, w_hh, b_ih, b_hh) re-laid out for the recurrent kernels (csrc/gru.hip); pack(p) refills the buffers
    in place (fill=False: allocate only)."""

    def __init__(self, p, H, D, fill=True):
        ub, hp, np_ = gru_dims(H)
        f = dict(device=p[0].device, dtype=torch.float32)
        self.UB, self.HP, self.NP, self.H, self.D = ub, hp, np_, H, D
        self.w_ihp = torch.empty((np_, D), **f)
        self.b_p = torch.empty(np_, **f)
        self.wf = torch.empty(ub * 3 * ub * 256, **f)
        self.wb = torch.empty(ub * (np_ // 16) * 256, **f)
        self.bufs = (self.w_ihp, self.b_p, self.wf, self.wb)
        if fill:
            self.pack(p)

    def pack(self, p):
        L.check(L.lib().nnr_gru_pack_weights(*[_p(t) for t in p], self.H, self.D, _p(self.w_ihp), _p(self.b_p), _p(self.wf), _p(self.wb), _s()),
                'nnr_gru_pack_weights')


def gru_pack(gru, H, D):
    """The parameters of `gru` (layers.GRUParams) in the recurrent kernels' layouts (GruPacked), behind the derived-weight cache with the
    freshness rule of the LSTM packs: refilled in place when a parameter changed."""
    p = gru.param_list()
    e = _derived('gru', gru, (H, D), lambda: GruPacked(p, H, D, fill=False), False)
    _serve(e, p, lambda: e.out.pack(p))
    return e.out


def gru_unpack_grads(dw_ihp, db_p, dw_hhp, H, D, grads):
    """grads: (w_ih, w_hh, b_ih, b_hh) gradients in nn.GRU's layout, added into without atomics."""
    L.check(L.lib().nnr_gru_unpack_grads(_p(dw_ihp), _p(db_p), _p(dw_hhp), H, D, *[_p(t) for t in grads], _s()), 'nnr_gru_unpack_grads')


def _gru_flops(B, T, H, cols):
    def flops(vals=None):
        return 2.0 * B * T * H * cols * H        # upper bound: every slot live
    flops.dyn = []
    flops.tag = 'B%d T%d H%d' % (B, T, H)
    return flops


def gru_fwd(gates, mask, h0, w, B, T, H, hout, hprev, hfinal, length):
    """rc of nnr_gru_fwd is checked; mask uint8 [B, T] contiguous."""
    assert mask.dtype == torch.uint8 and mask.is_contiguous()
    with _prof.span('gru_fwd', _gru_flops(B, T, H, 3)):
        L.check(L.lib().nnr_gru_fwd(_p(gates), _p(mask), _p(h0), _p(w.wf), B, T, H, _p(hout), _p(hprev), _p(hfinal), _p(length), _s()), 'nnr_gru_fwd')


def gru_bwd(gates, length, hprev, w, dhfinal, B, T, H, dh0=None):
    with _prof.span('gru_bwd', _gru_flops(B, T, H, 4)):
        L.check(L.lib().nnr_gru_bwd(_p(gates), _p(length), _p(hprev), _p(w.wb), _p(dhfinal), B, T, H, _p(dh0), _s()), 'nnr_gru_bwd')


def gru_zero_empty(y, length):
    B, D = y.shape
    L.check(L.lib().nnr_gru_zero_empty(_p(y), _p(length), B, D, _s()), 'nnr_gru_zero_empty')


def gru_tanh_bwd(dy, y, length, dz):
    B, D = y.shape
    L.check(L.lib().nnr_gru_tanh_bwd(_p(dy), _p(y), _p(length), B, D, _p(dz), _s()), 'nnr_gru_tanh_bwd')


# ---------------------------------------------------------------------------------------------- pooling
def _pool_args(x, ldx, D, n, Lx, plan=None, mask=None, mask_div=1, score=None, v=None, ldv=0, scale=1.0, alpha=None, out=None,
               ldo=0, add_in=None, ldadd=0, dout=None, lddo=0, dout2=None, lddo2=0, dx=None, lddx=0, dx_accumulate=False,
               dscore=None, dv=None, lddv=0, th=None, w2=None, alpha_b=None, dout_b=None, lddo_b=0, dscore_b=None, v_b=None, ldv_b=0, scale_b=1.0):
    a = L.PoolArgs()
    a.x, a.ldx, a.D, a.n, a.L = _p(x), ldx, D, n, Lx
    a.packed = int(plan is not None)
    if plan is not None:
        a.off, a.slen, a.order = _p(plan.off), _p(plan.slen), _p(plan.order)
    if mask is not None:
        a.mask = _p(mask.view(torch.uint8) if mask.dtype == torch.bool else mask)
    a.mask_div = mask_div
    a.score, a.v, a.ldv, a.scale, a.alpha = _p(score), _p(v), ldv, float(scale), _p(alpha)
    a.out, a.ldo, a.add_in, a.ldadd = _p(out), ldo, _p(add_in), ldadd
    a.dout, a.lddo, a.dout2, a.lddo2 = _p(dout), lddo, _p(dout2), lddo2
    a.dx, a.lddx, a.dx_accumulate, a.dscore, a.dv, a.lddv = _p(dx), lddx, int(dx_accumulate), _p(dscore), _p(dv), lddv
    if th is not None:            # forward: score = <th[row], w2> inside the pool's pass (instead of a separate nnr_rowdot launch)
        a.th, a.ldth, a.A, a.w2 = _p(th), th.stride(0), th.shape[1], _p(w2)
    if alpha_b is not None:       # backward: a second pool's token gradient folded into this call's one write of dx (csrc/pool.hip)
        a.alpha_b, a.dout_b, a.lddo_b, a.dscore_b, a.v_b, a.ldv_b, a.scale_b = _p(alpha_b), _p(dout_b), lddo_b, _p(dscore_b), _p(v_b), ldv_b, float(scale_b)
    return a


def _pool_span(family, kw, per_token_arrays):
    """x [tokens, D] is the operand that matters: forward reads it once (+ the tanh projection when the score is fused), backward
    reads it and writes dx (+ reads dx when it accumulates); per-sequence vectors are n x D."""
    if not _prof.active():
        return _NOSPAN
    plan, D, n, Lx = kw.get('plan'), kw['D'], kw['n'], kw['Lx']
    th = kw.get('th')
    per_row = 4.0 * (D * per_token_arrays + (th.shape[1] if th is not None else 0) + 2)
    return _hbm_span(family, per_row, n * Lx, dyn=plan.total if plan is not None else None, fixed=4.0 * n * D * 3)


def pool_fwd(**kw):
    with _pool_span('pool_fwd', kw, 1):
        L.check(L.lib().nnr_attn_pool_fwd(C.byref(_pool_args(**kw)), _s()), 'nnr_attn_pool_fwd')


def pool_bwd(**kw):
    with _pool_span('pool_bwd', kw, (3 if kw.get('dx_accumulate') else 2) if kw.get('dx') is not None else 1):
        L.check(L.lib().nnr_attn_pool_bwd(C.byref(_pool_args(**kw)), _s()), 'nnr_attn_pool_bwd')


# ---------------------------------------------------------------------------------------------- elementwise
def add_(y, x, alpha=1.0):
    assert y.is_contiguous() and x.is_contiguous() and y.numel() == x.numel()
    L.check(L.lib().nnr_add(_p(y), _p(x), y.numel(), alpha, _s()), 'nnr_add')
    return y


def add_atomic_(y, x, alpha=1.0):
    assert y.is_contiguous() and x.is_contiguous() and y.numel() == x.numel()
    L.check(L.lib().nnr_add_atomic(_p(y), _p(x), y.numel(), alpha, _s()), 'nnr_add_atomic')
    return y


def expand_rows(x, N):
    """[B, D] -> [B, N, D]: x repeated over N (userEncoders.py:172,190), one launch."""
    B, D = x.shape
    y = torch.empty((B, N, D), device=x.device, dtype=torch.float32)
    L.check(L.lib().nnr_expand_rows_fwd(_p(x), _p(y), B, N, D, _s()), 'nnr_expand_rows_fwd')
    return y


def expand_rows_bwd(dy):
    """[B, N, D] -> [B, D]: the sum over N in ascending order, one launch."""
    B, N, D = dy.shape
    dx = torch.empty((B, D), device=dy.device, dtype=torch.float32)
    L.check(L.lib().nnr_expand_rows_bwd(_p(dy), _p(dx), B, N, D, _s()), 'nnr_expand_rows_bwd')
    return dx


def add2d(y, ldy, x, ldx, rows, cols, alpha=1.0, accumulate=False):
    L.check(L.lib().nnr_add2d(_p(y), ldy, _p(x), ldx, rows, cols, alpha, accumulate, _s()), 'nnr_add2d')


def gate_bwd(dHt, H, G, dH, dpre, plan, cols):
    with _hbm_span('gate_bwd', 5 * 4.0 * cols, plan.cap, dyn=plan.total):      # reads dHt, H, G; writes dH, dpre
        return _gate_bwd(dHt, H, G, dH, dpre, plan, cols)


def _gate_bwd(dHt, H, G, dH, dpre, plan, cols):
    L.check(L.lib().nnr_gate_bwd(_p(dHt), _p(H), _p(G), _p(dH), _p(dpre), _p(plan.total), plan.cap, cols, _s()), 'nnr_gate_bwd')


def packed_seq_sum(x, D, plan, out):
    L.check(L.lib().nnr_packed_seq_sum(_p(x), D, _p(plan.off), _p(plan.slen), plan.n, _p(out), _s()), 'nnr_packed_seq_sum')


def tanh_score_bwd(th, ds, w2, dw2, plan, A):
    rows = plan.cap if plan is not None else th.shape[0]
    ws = _slot_ws(th.device, A)                  # (reproducible dw2: see csrc/misc.hip slot_reduce_kernel)
    L.check(L.lib().nnr_tanh_score_bwd(_p(th), _p(ds), _p(w2), _p(dw2), _p(plan.total) if plan is not None else None, rows, A, _p(ws),
                                       _s()), 'nnr_tanh_score_bwd')


def small_embed_fwd(table, idx, out_view, ldo, p, seed):
    n, dim = idx.numel(), table.shape[1]
    L.check(L.lib().nnr_small_embed_fwd(_p(table), _p(idx), n, dim, _p(out_view), ldo, p, seed, _s()), 'nnr_small_embed_fwd')


def small_embed_bwd(idx, dim, dout_view, lddo, dtable, p, seed):
    L.check(L.lib().nnr_small_embed_bwd(_p(idx), idx.numel(), dim, _p(dout_view), lddo, _p(dtable), p, seed, _s()), 'nnr_small_embed_bwd')


def dropout(x, p, seed, out=None):
    if out is None:
        out = torch.empty_like(x)
    L.check(L.lib().nnr_dropout(_p(x), _p(out), x.numel(), p, seed, _s()), 'nnr_dropout')
    return out


def layernorm_fwd(u, gamma, beta, eps, xhat, rstd, r_out, resid, y, p, seed):
    """y = dropout(relu(LayerNorm(u) * gamma + beta) + resid) over the last dimension of a contiguous [rows, D] u."""
    rows, D = u.numel() // u.shape[-1], u.shape[-1]
    L.check(L.lib().nnr_layernorm_fwd(_p(u), _p(gamma), _p(beta), eps, rows, D, _p(xhat), _p(rstd), _p(r_out), _p(resid), _p(y), p, seed, _s()),
                                      'nnr_layernorm_fwd')


def layernorm_bwd(dv, xhat, rstd, gamma, du, dgamma, dbeta):
    rows, D = dv.numel() // dv.shape[-1], dv.shape[-1]
    L.check(L.lib().nnr_layernorm_bwd(_p(dv), _p(xhat), _p(rstd), _p(gamma), rows, D, _p(du), _p(dgamma), _p(dbeta), _s()), 'nnr_layernorm_bwd')


def relu_bwd(dy, y, dx=None):
    if dx is None:
        dx = torch.empty_like(dy)
    L.check(L.lib().nnr_relu_bwd(_p(dy), _p(y), _p(dx), dy.numel(), _s()), 'nnr_relu_bwd')
    return dx


def relu_drop_bwd(dy, r, ds, dx, p, seed):
    L.check(L.lib().nnr_relu_drop_bwd(_p(dy), _p(r), _p(ds), _p(dx), dy.numel(), p, seed, _s()), 'nnr_relu_drop_bwd')


def sigmoid_drop_bwd(dy, s, dz, p, seed):
    """dz = mask(dy) * s * (1 - s): backward of y = dropout(sigmoid(z)) given s = sigmoid(z)."""
    L.check(L.lib().nnr_sigmoid_drop_bwd(_p(dy), _p(s), _p(dz), dy.numel(), p, seed, _s()), 'nnr_sigmoid_drop_bwd')


# ---------------------------------------------------------------------------------------------- SUE / loss / optimiser
def gcn_aggregate_fwd(graph, z, bias, resid, r_out, y, B, G, D, relu, p, seed):
    arrays = 3 + (1 if resid is not None else 0)                                  # z, (resid) read; r, y written
    with _hbm_span('gcn_aggregate_fwd', 4.0 * (G * D * arrays + G * G), B):
        L.check(L.lib().nnr_gcn_aggregate_fwd(_p(graph), _p(z), _p(bias), _p(resid), _p(r_out), _p(y), B, G, D, relu, p, seed, _s()),
                                              'nnr_gcn_aggregate_fwd')


def gcn_aggregate_bwd(graph, dy, r, ds, dx0, dz, B, G, D, p, seed):
    arrays = 4 + (1 if dx0 is not None else 0)                                    # dy, r read; dS, dz, (dx0) written
    with _hbm_span('gcn_aggregate_bwd', 4.0 * (G * D * arrays + G * G), B):
        L.check(L.lib().nnr_gcn_aggregate_bwd(_p(graph), _p(dy), _p(r), _p(ds), _p(dx0), _p(dz), B, G, D, p, seed, _s()), 'nnr_gcn_aggregate_bwd')


def sue_x0_fwd(hist, proxy, x0, B, Hn, Kc, D, p, seed, cmask_fix=None):
    """cmask_fix: the [B, Kc + 1] cluster mask; its last column is set in place by the same launch (userEncoders.py:73)."""
    if cmask_fix is not None:
        assert cmask_fix.is_contiguous() and cmask_fix.element_size() == 1 and tuple(cmask_fix.shape) == (B, Kc + 1)
    L.check(L.lib().nnr_sue_x0_fwd(_p(hist), _p(proxy), _p(x0), B, Hn, Kc, D, p, seed, _p(cmask_fix), _s()), 'nnr_sue_x0_fwd')


def sue_x0_bwd(dx0, dhist, dproxy, B, Hn, Kc, D, p, seed, dx0_add=None):
    L.check(L.lib().nnr_sue_x0_bwd(_p(dx0), _p(dx0_add), _p(dhist), _p(dproxy), B, Hn, Kc, D, p, seed, _s()), 'nnr_sue_x0_bwd')


def sue_slice_fwd(gcn, x0, gfeat, B, Hn, G, D):
    L.check(L.lib().nnr_sue_slice_fwd(_p(gcn), _p(x0), _p(gfeat), B, Hn, G, D, _s()), 'nnr_sue_slice_fwd')


def sue_slice_bwd(dgfeat, dpad, B, Hn, G, D):
    L.check(L.lib().nnr_sue_slice_bwd(_p(dgfeat), _p(dpad), B, Hn, G, D, _s()), 'nnr_sue_slice_bwd')


def sue_intra_fwd(kf, qc, g, cidx, B, N, Hn, Cn, A, D, alpha, feat):
    # per user: keys [Hn, A] + queries [N, A] + features [Hn, D] + indices read; weights [N, Hn] + cluster features [N, Cn, D] written
    with _hbm_span('sue_intra_fwd', 4.0 * (Hn * A + N * A + Hn * D + N * Hn + N * Cn * D) + 8.0 * Hn, B):
        return _sue_intra_fwd(kf, qc, g, cidx, B, N, Hn, Cn, A, D, alpha, feat)


def _sue_intra_fwd(kf, qc, g, cidx, B, N, Hn, Cn, A, D, alpha, feat):
    L.check(L.lib().nnr_sue_intra_fwd(_p(kf), _p(qc), _p(g), _p(cidx), B, N, Hn, Cn, A, D, _p(alpha), _p(feat), _s()), 'nnr_sue_intra_fwd')


def sue_intra_bwd(kf, qc, g, cidx, alpha, dfeat, B, N, Hn, Cn, A, D, dg, dkf, dqc):
    ws = torch.empty(B * N * Hn, device=kf.device, dtype=torch.float32)
    # per user: d cluster features [N, Cn, D], features [Hn, D], keys, queries, weights read; d features [Hn, D], d keys, d queries written
    with _hbm_span('sue_intra_bwd', 4.0 * (N * Cn * D + 2 * Hn * D + 2 * Hn * A + 2 * N * A + N * Hn) + 8.0 * Hn, B):
        return _sue_intra_bwd(kf, qc, g, cidx, alpha, dfeat, B, N, Hn, Cn, A, D, dg, dkf, dqc, ws)


def _sue_intra_bwd(kf, qc, g, cidx, alpha, dfeat, B, N, Hn, Cn, A, D, dg, dkf, dqc, ws):
    L.check(L.lib().nnr_sue_intra_bwd(_p(kf), _p(qc), _p(g), _p(cidx), _p(alpha), _p(dfeat), B, N, Hn, Cn, A, D, _p(dg), _p(dkf), _p(dqc),
                                      _p(ws), _s()), 'nnr_sue_intra_bwd')


SEG_POOL_MAXH, SEG_POOL_MAXC, SEG_POOL_MAXN = 64, 32, 8      # SUE_MAXH / SUE_MAXC / SUE_MAXN of csrc/sue_cluster.hip, for the constructors
SEG_POOL_UNSUPPORTED = 'unsupported size (the segmented candidate pool takes 1 <= history slots <= 64, 1 <= clusters <= 32 and 1 <= candidates <= 8)'


def seg_pool_supported(Hn, Cn, N=1, D=1, B=1):
    """The one host mirror of sue_cluster_ok (csrc/sue_cluster.hip), the size rule of nnr_sue_seg_pool_* and nnr_sue_intra_* (which also
    want A >= 1): no library call, no device."""
    return int(B) >= 1 and 1 <= int(N) <= SEG_POOL_MAXN and 1 <= int(Hn) <= SEG_POOL_MAXH and 1 <= int(Cn) <= SEG_POOL_MAXC and int(D) >= 1


def sue_seg_pool_fwd(x, u, cidx, B, N, Hn, Cn, D, scale, alpha, feat):
    """x [B, Hn, D], u [B*N, D], cidx int64 [B, Hn] -> alpha [B, N, Hn], feat [B*N*Cn, D]: the intra-cluster attention of SUE_wo_GCN with the
    key projection folded into the query (u = q W_K)."""
    L.check(L.lib().nnr_sue_seg_pool_fwd(_p(x), _p(u), _p(cidx), B, N, Hn, Cn, D, scale, _p(alpha), _p(feat), _s()), 'nnr_sue_seg_pool_fwd',
            SEG_POOL_UNSUPPORTED)


def sue_seg_pool_bwd(x, u, cidx, alpha, dfeat, B, N, Hn, Cn, D, scale, dx, du):
    """dx [B, Hn, D] is written (not accumulated), du [B*N, D] too."""
    if not seg_pool_supported(Hn, Cn, N, D, B):          # (before the scratch allocation, whose size the arguments give)
        raise L.NnrHipError('nnr_sue_seg_pool_bwd: ' + SEG_POOL_UNSUPPORTED)
    ws = torch.empty(B * N * Hn, device=x.device, dtype=torch.float32)
    L.check(L.lib().nnr_sue_seg_pool_bwd(_p(x), _p(u), _p(cidx), _p(alpha), _p(dfeat), B, N, Hn, Cn, D, scale, _p(dx), _p(du), _p(ws), _s()),
            'nnr_sue_seg_pool_bwd', SEG_POOL_UNSUPPORTED)


def _u8(mask):
    return None if mask is None else (mask.view(torch.uint8) if mask.dtype == torch.bool else mask)


def mask_u8(mask):
    """`mask` as the contiguous uint8 tensor the kernels read: a bool or uint8 mask is viewed, any other dtype compared with 0; None stays."""
    return None if mask is None else _u8(mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()


def ids32(ids, *shape):
    """`ids` as a contiguous int32 tensor of `shape` (int32 already: no conversion; contiguous already: no copy)."""
    return (ids if ids.dtype == torch.int32 else ids.to(torch.int32)).reshape(shape).contiguous()


def cand_attn_fwd(P, Q, w2, feat, mask, B, N, H, A, D, act, alpha, out):
    """Candidate-aware additive attention (csrc/cand_attn.hip): P [B*N, A], Q [B*H, A], w2 [A], feat [B, H, D], mask [B, H] bool / uint8 or
    None -> alpha [B, N, H], out [B, N, D]."""
    # per sample: both projections + features + mask read; weights [N, H] + outputs [N, D] written
    with _hbm_span('cand_attn_fwd', 4.0 * (N * A + H * A + H * D + N * H + N * D) + 1.0 * H, B, fixed=4.0 * A):
        L.check(L.lib().nnr_cand_attn_fwd(_p(P), _p(Q), _p(w2), _p(feat), feat.stride(1), _p(_u8(mask)), B, N, H, A, D, act, _p(alpha), _p(out),
                                          _s()), 'nnr_cand_attn_fwd')


def cand_attn_bwd(P, Q, w2, feat, mask, alpha, dout, B, N, H, A, D, act, dP, dQ, dfeat, dw2, accumulate=False):
    """dP [B*N, A], dQ [B*H, A], dfeat [B, H, D] (added into when `accumulate`) are written, dw2 [A] is added into."""
    ws = torch.empty(L.lib().nnr_cand_attn_ws_floats(B, N, H, A), device=P.device, dtype=torch.float32)
    # per sample: projections, features, weights, d outputs read; d projections, d features written (+ the workspace's da and dw2 rows, both ways)
    with _hbm_span('cand_attn_bwd', 4.0 * (2 * N * A + 2 * H * A + (3 if accumulate else 2) * H * D + 3 * N * H + N * D + 2 * N * A) + 1.0 * H, B,
                   fixed=8.0 * A):
        L.check(L.lib().nnr_cand_attn_bwd(_p(P), _p(Q), _p(w2), _p(feat), feat.stride(1), _p(_u8(mask)), _p(alpha), _p(dout), B, N, H, A, D, act,
                                          _p(dP), _p(dQ), _p(dfeat), accumulate, _p(ws), _p(dw2), _s()), 'nnr_cand_attn_bwd')


def pers_attn_fwd(Qf, P, uidx, w2, feat, mask, n, Lx, A, F, alpha, out, U=None):
    """Per-title personalised attention (csrc/pers_attn.hip): Qf [n*L, A], P [U, A], uidx int32 [n], w2 [A], feat [n, L, F], mask [n, L] bool /
    uint8 or None -> alpha [n, L], out [n, F].  Returns the entry point's code for NNR_ERR_UNSUPPORTED (-3) instead of raising."""
    U = P.shape[0] if U is None else U
    # per title: the projection rows and feature rows of its live positions (counted as all L), weights + output written; P and w2 once per user
    with _hbm_span('pers_attn_fwd', 4.0 * (Lx * A + Lx * F + Lx + F) + 1.0 * Lx + 4.0, n, fixed=4.0 * A * (U + 1)):
        rc = L.lib().nnr_pers_attn_fwd(_p(Qf), _p(P), _p(uidx), U, _p(w2), _p(feat), feat.stride(1), _p(_u8(mask)), n, Lx, A, F, _p(alpha), _p(out), _s())
    if rc == -3:
        return rc
    L.check(rc, 'nnr_pers_attn_fwd')
    return 0


def pers_attn_bwd(Qf, P, uidx, w2, feat, mask, alpha, dout, n, Lx, A, F, dP, dQf, dfeat, dw2, U=None):
    """dP [U, A], dQf [n*L, A], dfeat [n, L, F] are written, dw2 [A] is added into."""
    U = dP.shape[0] if U is None else U
    nws = L.lib().nnr_pers_attn_ws_floats(n, Lx, A)
    if nws < 0:
        raise L.NnrHipError('nnr_pers_attn_ws_floats failed with code %d (n %d, L %d, A %d)' % (nws, n, Lx, A))
    ws = torch.empty(nws, device=Qf.device, dtype=torch.float32)
    # per title: projection rows + feature rows read, their gradients written, weights, d output, the two workspace rows (both ways)
    with _hbm_span('pers_attn_bwd', 4.0 * (2 * Lx * A + 2 * Lx * F + Lx + F + 4 * A) + 1.0 * Lx + 4.0, n, fixed=4.0 * A * (2 * U + 2)):
        L.check(L.lib().nnr_pers_attn_bwd(_p(Qf), _p(P), _p(uidx), U, _p(w2), _p(feat), feat.stride(1), _p(_u8(mask)), _p(alpha), _p(dout), n, Lx, A,
                                          F, _p(dP), _p(dQf), _p(dfeat), _p(ws), _p(dw2), _s()), 'nnr_pers_attn_bwd')


def user_rows_fwd(table, ids, p, seed, rows=None):
    """out[b] = dropout(table[ids[b]]) for int64 ids [B] (csrc/misc.hip); an id outside [0, rows) gives a zero row."""
    B, dim = ids.numel(), table.shape[1]
    out = torch.empty((B, dim), device=table.device, dtype=torch.float32)
    L.check(L.lib().nnr_user_rows_fwd(_p(table), table.shape[0] if rows is None else rows, _p(ids), B, dim, _p(out), p, seed, _s()), 'nnr_user_rows_fwd')
    return out


def user_rows_bwd(dout, ids, dtable, p, seed, rows=None):
    """dtable[u] += sum over b with ids[b] == u, in ascending b, of mask * dout[b] (no float atomics)."""
    B, dim = ids.numel(), dtable.shape[1]
    L.check(L.lib().nnr_user_rows_bwd(_p(dout), _p(ids), B, dtable.shape[0] if rows is None else rows, dim, _p(dtable), p, seed, _s()), 'nnr_user_rows_bwd')


def omap_ws(B, N, H, D, K, device):
    n = L.lib().nnr_omap_ws_floats(B, N, H, D, K)
    if n < 0:
        raise L.NnrHipError('nnr_omap_ws_floats failed with code %d (B %d, N %d, H %d, D %d, K %d)' % (n, B, N, H, D, K))
    return torch.empty(n, device=device, dtype=torch.float32)


def omap_fwd(hist, cand, mask, W, B, N, H, D, K, alpha, Y, beta, R, gamma, out):
    """The OMAP user encoder (csrc/omap.hip): hist [B, H, D] (row stride allowed), cand [B, N, D], mask [B, H] bool / uint8 or None, W [D, K]
    -> alpha [B, H, H], Y [B, H, D], beta [B, H, K], R [B, K, D], gamma [B, N, K], out [B, N, D]."""
    ws = omap_ws(B, N, H, D, K, hist.device)
    # per user: X read by the score and the mix launch, alpha written and read, Y written and read, candidates, archives (written, read),
    # outputs, the small tensors; W once
    with _hbm_span('omap_fwd', 4.0 * (2 * H * D + 2 * H * H + 2 * H * D + N * D + 2 * K * D + N * D + 2 * H * K + N * K) + 1.0 * H, B,
                   fixed=4.0 * D * K):
        L.check(L.lib().nnr_omap_fwd(_p(hist), hist.stride(1), _p(cand), _p(_u8(mask)), _p(W), B, N, H, D, K, _p(alpha), _p(Y), _p(beta), _p(R),
                                     _p(gamma), _p(out), _p(ws), _s()), 'nnr_omap_fwd')


def omap_bwd(hist, cand, mask, W, alpha, Y, beta, R, gamma, dout, B, N, H, D, K, dhist, dcand, dW, accumulate=False):
    """dhist [B, H, D] (added into when `accumulate`) and dcand [B, N, D] are written, dW [D, K] is added into."""
    ws = omap_ws(B, N, H, D, K, hist.device)
    # per user: X twice, Y twice, alpha twice, G both ways, d outputs + candidates + archives, dR both ways (read twice), d candidates,
    # d history (read first when it accumulates), the user's dW rows both ways
    with _hbm_span('omap_bwd', 4.0 * (2 * H * D + 2 * H * D + 2 * H * H + 2 * H * H + 2 * N * D + K * D + 3 * K * D + N * D +
                                      (2 if accumulate else 1) * H * D + 2 * D * K + 3 * H * K) + 1.0 * H, B, fixed=12.0 * D * K):
        L.check(L.lib().nnr_omap_bwd(_p(hist), hist.stride(1), _p(cand), _p(_u8(mask)), _p(W), _p(alpha), _p(Y), _p(beta), _p(R), _p(gamma), _p(dout),
                                     B, N, H, D, K, _p(dhist), accumulate, _p(dcand), _p(dW), _p(ws), _s()), 'nnr_omap_bwd')


def omap_reg_fwd(W, coef, off, loss):
    """loss (0-dim) = coef * ||(W^T W) o (J - I)||_F; off [K * K + 1] keeps the off-diagonal part and the norm for omap_reg_bwd."""
    D, K = W.shape
    L.check(L.lib().nnr_omap_reg_fwd(_p(W), D, K, coef, _p(off), _p(loss), _s()), 'nnr_omap_reg_fwd')


def omap_reg_bwd(W, off, gup, coef, dW):
    """dW += gup * coef * 2 W Off / Omega (gup: 0-dim device tensor; nothing at Omega == 0)."""
    D, K = W.shape
    L.check(L.lib().nnr_omap_reg_bwd(_p(W), _p(off), _p(gup), D, K, coef, _p(dW), _s()), 'nnr_omap_reg_bwd')


def logits_loss_fwd(user, cand, B, N, D, logits, loss, dlogits):
    L.check(L.lib().nnr_logits_loss_fwd(_p(user), _p(cand), B, N, D, _p(logits), _p(loss), _p(dlogits), _s()), 'nnr_logits_loss_fwd')


def logits_fwd(user, cand, B, N, D, logits):
    L.check(L.lib().nnr_logits_fwd(_p(user), _p(cand), B, N, D, _p(logits), _s()), 'nnr_logits_fwd')


def list_scores(user, reps, row, cand, scores=None, check=True):
    """scores[j] = <user[row[j]], reps[cand[j]]> (nnr_list_scores; its summation order is stated in include/nnr_hip.h): user [n_user, D] and
    reps [n_reps, D] float32 with unit column stride (any row stride >= D), row / cand int32 [n] -> float32 [n] (written into `scores` when
    given; entries beyond n stay).  The kernel trusts the indices: check=True reads their ranges back (two reductions, one sync) and raises
    before the launch."""
    n_user, n_reps, D, ldu, ldr = _pool_tables('list_scores', user, reps, None, None)[:5]
    n = row.numel()
    if row.dtype != torch.int32 or cand.dtype != torch.int32 or cand.numel() != n or not (row.is_contiguous() and cand.is_contiguous()):
        raise L.NnrHipError('list_scores: row and cand must be contiguous int32 tensors of one length')
    if n < 1:
        raise L.NnrHipError('list_scores: empty input (no row / cand pairs)')
    if scores is None:
        scores = torch.empty(n, device=user.device, dtype=torch.float32)
    elif scores.dtype != torch.float32 or scores.numel() < n or not scores.is_contiguous():
        raise L.NnrHipError('list_scores: scores must be a contiguous float32 tensor of at least n entries')
    if check:
        _p(row), _p(cand)
        lo_r, hi_r, lo_c, hi_c = torch.stack(torch.aminmax(row) + torch.aminmax(cand)).tolist()
        if lo_r < 0 or hi_r >= n_user or lo_c < 0 or hi_c >= n_reps:
            raise L.NnrHipError('list_scores: row indices %d..%d for %d user rows, cand indices %d..%d for %d news rows'
                                % (lo_r, hi_r, n_user, lo_c, hi_c, n_reps))
    L.check(L.lib().nnr_list_scores(_p(user), n_user, ldu, _p(reps), n_reps, ldr, _p(row), _p(cand), n, D, _p(scores), _s()), 'nnr_list_scores')
    return scores


_TOPK_WS = {}


def _topk_ws(dev, nbytes):
    """Partial-list workspace of the CURRENT stream (nnr_topk_workspace_bytes): the tile launch fills it and the merge launch behind it on
    the same stream reads it, so the calls of one stream share one buffer, grown when a bigger launch comes along."""
    if nbytes == 0:
        return None
    key = torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    ws = _TOPK_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
        _TOPK_WS[key] = ws
    tape_keep(ws)
    return ws


def _pool_tables(name, user, reps, valid, exclude):
    """The argument checks list_scores, topk_scores and pool_ranks share, before anything is launched: (n_user, n_reps, D, ldu, ldr, exclude, E,
    ld_ex)."""
    if user.dim() != 2 or reps.dim() != 2 or reps.shape[1] != user.shape[1] or user.dtype != torch.float32 or reps.dtype != torch.float32:
        raise L.NnrHipError('%s: user [n_user, D] and reps [n_reps, D] must be float32 tables of one width' % name)
    (n_user, D), n_reps = user.shape, reps.shape[0]
    if n_user < 1 or n_reps < 1 or D < 1 or (D > 1 and (user.stride(1) != 1 or reps.stride(1) != 1)):
        raise L.NnrHipError('%s: empty input or a table whose columns are not adjacent' % name)
    if valid is not None and (valid.dtype not in (torch.bool, torch.uint8) or valid.dim() != 1 or valid.numel() != n_reps
                              or not valid.is_contiguous()):
        raise L.NnrHipError('%s: valid must be a contiguous bool / uint8 vector of one entry per row of reps (%d)' % (name, n_reps))
    E = ld_ex = 0
    if exclude is not None:
        if exclude.dtype != torch.int32 or exclude.dim() != 2 or exclude.shape[0] != n_user or (exclude.shape[1] > 1 and exclude.stride(1) != 1):
            raise L.NnrHipError('%s: exclude must be int32 [n_user = %d, E] with adjacent columns' % (name, n_user))
        E = exclude.shape[1]
        ld_ex = exclude.stride(0) if n_user > 1 else E
        if E == 0:
            exclude = None
        elif ld_ex < E:
            raise L.NnrHipError('%s: exclude rows overlap (row stride %d for %d entries)' % (name, ld_ex, E))
    ldu = user.stride(0) if n_user > 1 else D
    ldr = reps.stride(0) if n_reps > 1 else D
    if ldu < D or ldr < D:
        raise L.NnrHipError('%s: overlapping rows (row strides %d, %d for width %d)' % (name, ldu, ldr, D))
    return n_user, n_reps, D, ldu, ldr, exclude, E, ld_ex


_NOT_FINITE = '%s: user and reps must be finite (a NaN or an infinity leaves the order undefined)'


def _tables_finite(user, reps):
    """0-dim device bool: both tables are finite (two reductions where they live; the caller reads it back, alone or with its other flags)."""
    return torch.isfinite(user).all() & torch.isfinite(reps).all()


def _archive_tables(name, user, reps, valid, exclude, archives, lda):
    """The archive form's user table (nnr_topk_archive_scores, include/nnr_hip.h) as _pool_tables sees it: `user` is [n_user, A, D] (unit
    stride along D, any stride lda >= D between archives) or [n_user, >= (A - 1) * lda + D] with archive a of a row at columns a * lda ..
    (lda defaults to D).  Returns (_pool_tables' tuple with the archive-aware ldu, lda, the [n_user, A, D] view that the launch reads)."""
    A = archives
    if not isinstance(A, int) or isinstance(A, bool) or A < 1:
        raise L.NnrHipError('%s: archives = %r (an integer from 1 to 16)' % (name, A))
    D = reps.shape[1] if reps.dim() == 2 else -1
    if user.dim() == 3 and tuple(user.shape[1:]) == (A, D) and lda in (None, user.stride(1)):
        lda = user.stride(1) if A > 1 else D
        first = user[:, 0, :]
    elif user.dim() == 2 and D >= 1 and (D if lda is None else lda) >= D and user.shape[1] >= (A - 1) * (D if lda is None else lda) + D:
        lda = D if lda is None else int(lda)
        first = user[:, :D]
    else:
        raise L.NnrHipError('%s: with archives = %d the user table is [n_user, %d, D] or [n_user, (archives - 1) * lda + D and more] with '
                            'lda >= D = the width of reps (got %r, lda %r, reps %r)' % (name, A, A, tuple(user.shape), lda, tuple(reps.shape)))
    t = _pool_tables(name, first, reps, valid, exclude)
    n_user, D, ldu = t[0], t[2], t[3]
    if n_user == 1:
        ldu = (A - 1) * lda + D
    if lda < D or ldu < (A - 1) * lda + D:
        raise L.NnrHipError('%s: overlapping archives (lda %d, row stride %d for %d archives of width %d)' % (name, lda, ldu, A, D))
    return t[:3] + (ldu,) + t[4:], lda, first.as_strided((n_user, A, D), (ldu, lda, 1))


def _archive_scale(name, scale):
    scale = float(scale)
    if scale != scale or scale in (float('inf'), float('-inf')):
        raise L.NnrHipError('%s: scale = %r is not finite' % (name, scale))
    return scale


_ARCHIVES_UNSUPPORTED = 'archives = %d is unsupported beyond 16 (the OMAP kernels\' own limit on their archives); '


def topk_scores(user, reps, K, valid=None, exclude=None, check=True, archives=1, lda=None, scale=0.0):
    """(idx int32 [n_user, K], score float32 [n_user, K]): for every user row the K eligible rows of `reps` with the largest <user, reps row>,
    by score descending, equal scores by ascending row; idx = -1 / score = -inf where fewer than K rows are eligible (nnr_topk_scores,
    include/nnr_hip.h, which states the summation order).  user [n_user, D] and reps [n_reps, D] float32 with unit column stride (any row stride
    >= D); valid: bool / uint8 [n_reps], nonzero = in the pool, or None; exclude: int32 [n_user, E] (unit column stride) of rows a user must
    not get, entries outside 0 .. n_reps - 1 (a -1 pad) ignored, or None.  1 <= K <= 64.  The [n_user, n_reps] scores never exist.  The
    tables are finite by contract: check=True verifies that (two reductions, one sync) and raises before the launch.
    archives = A > 1 (or a 3-D user table): the archive form, nnr_topk_archive_scores -- a user row is A vectors ([n_user, A, D], or
    [n_user, A * D] with the archives `lda` = D columns apart) and the score of a pair is sum_a w_a <user[u, a], reps row> with
    w = softmax_a(scale * <user[u, a], reps row>), by the operation sequence the header states.  With archives == 1 and a 2-D table the
    plain entry point is called, exactly as without these keywords."""
    arch = type(archives) is not int or archives != 1 or user.dim() == 3
    if arch:
        (n_user, n_reps, D, ldu, ldr, exclude, E, ld_ex), lda, user = _archive_tables('topk_scores', user, reps, valid, exclude, archives, lda)
        scale = _archive_scale('topk_scores', scale)
    else:
        n_user, n_reps, D, ldu, ldr, exclude, E, ld_ex = _pool_tables('topk_scores', user, reps, valid, exclude)
    if not isinstance(K, int) or K < 1:
        raise L.NnrHipError('topk_scores: K = %r (an integer from 1 to 64)' % (K,))
    _p(user), _p(reps), _p(valid), _p(exclude)
    if check and not bool(_tables_finite(user, reps)):
        raise L.NnrHipError(_NOT_FINITE % 'topk_scores')
    idx = torch.empty((n_user, K), device=user.device, dtype=torch.int32)
    score = torch.empty((n_user, K), device=user.device, dtype=torch.float32)
    nbytes = L.lib().nnr_topk_workspace_bytes(n_user, n_reps, K)
    ws = _topk_ws(user.device, nbytes)
    if arch:
        L.check(L.lib().nnr_topk_archive_scores(_p(user), n_user, ldu, archives, lda, scale, _p(reps), n_reps, ldr, D, _p(_u8(valid)), _p(exclude),
                                                E, ld_ex, K, _p(idx), _p(score), _p(ws), nbytes, _s()), 'nnr_topk_archive_scores',
                unsupported=_ARCHIVES_UNSUPPORTED % archives + 'so are K = %d beyond 64 and 2^31 news rows and more' % K)
        return idx, score
    L.check(L.lib().nnr_topk_scores(_p(user), n_user, ldu, _p(reps), n_reps, ldr, D, _p(_u8(valid)), _p(exclude), E, ld_ex, K, _p(idx), _p(score),
                                    _p(ws), nbytes, _s()), 'nnr_topk_scores', unsupported='K = %d is unsupported beyond 64 (a running list is one entry per lane of a wave), as are 2^31 news rows and more' % K)
    return idx, score


def pool_ranks(user, reps, t_off, t_news, valid=None, exclude=None, check=True, archives=1, lda=None, scale=0.0):
    """(ahead int32 [T], t_score float32 [T], pool_size int32 [n_user]): where the targets land when each user's whole pool is ranked
    (nnr_pool_ranks, include/nnr_hip.h).  user, reps, valid and exclude as for topk_scores, with its eligibility rule.  t_off: int32
    [n_user + 1], non-decreasing from 0 to T; t_news: int32 [T], rows of `reps`; entries t_off[u] .. t_off[u + 1] - 1 are the targets of user
    row u (none, many, repeats).  ahead[j] = the number of eligible rows that topk_scores would place before target j (greater score, or equal
    score and smaller row), -1 when the target is itself ineligible for its user; t_score[j] = its score, with the bits topk_scores returns;
    pool_size[u] = the user's eligible rows.  check=True verifies that the tables are finite, t_off is ordered from 0 to T and t_news lies
    inside the table (reductions on the device, one sync) and raises before the launch.  archives, lda, scale: the archive form
    (nnr_pool_archive_ranks), with topk_scores' table layout and score; archives == 1 with a 2-D table calls the plain entry point."""
    arch = type(archives) is not int or archives != 1 or user.dim() == 3
    if arch:
        (n_user, n_reps, D, ldu, ldr, exclude, E, ld_ex), lda, user = _archive_tables('pool_ranks', user, reps, valid, exclude, archives, lda)
        scale = _archive_scale('pool_ranks', scale)
    else:
        n_user, n_reps, D, ldu, ldr, exclude, E, ld_ex = _pool_tables('pool_ranks', user, reps, valid, exclude)
    if (t_off.dtype != torch.int32 or t_news.dtype != torch.int32 or t_off.dim() != 1 or t_news.dim() != 1
            or not (t_off.is_contiguous() and t_news.is_contiguous())):
        raise L.NnrHipError('pool_ranks: t_off and t_news must be contiguous int32 vectors')
    T = t_news.numel()
    if t_off.numel() != n_user + 1:
        raise L.NnrHipError('pool_ranks: t_off has %d entries for %d user rows (one more than rows)' % (t_off.numel(), n_user))
    if check:                                               # three reductions where the tensors live, one read-back
        bad_off = (t_off[0] != 0) | (t_off[-1] != T) | (t_off[1:] < t_off[:-1]).any()
        bad_news = ((t_news < 0) | (t_news >= n_reps)).any() if T else torch.zeros_like(bad_off)
        bad_off, bad_news, finite = torch.stack([bad_off.to(user.device), bad_news.to(user.device), _tables_finite(user, reps)]).tolist()
        if bad_off:
            raise L.NnrHipError('pool_ranks: t_off must be non-decreasing from 0 to the number of targets (%d)' % T)
        if bad_news:
            raise L.NnrHipError('pool_ranks: t_news outside 0 .. %d (the rows of reps)' % (n_reps - 1))
        if not finite:
            raise L.NnrHipError(_NOT_FINITE % 'pool_ranks')
    _p(user), _p(reps), _p(valid), _p(exclude), _p(t_off), _p(t_news)
    dev = user.device
    ahead = torch.empty(T, device=dev, dtype=torch.int32)
    t_score = torch.empty(T, device=dev, dtype=torch.float32)
    pool_size = torch.empty(n_user, device=dev, dtype=torch.int32)
    nbytes = L.lib().nnr_pool_rank_workspace_bytes(n_user, n_reps, T)
    ws = _topk_ws(dev, nbytes)
    if arch:
        L.check(L.lib().nnr_pool_archive_ranks(_p(user), n_user, ldu, archives, lda, scale, _p(reps), n_reps, ldr, D, _p(_u8(valid)), _p(exclude),
                                               E, ld_ex, _p(t_off), _p(t_news) if T else None, T, _p(ahead) if T else None,
                                               _p(t_score) if T else None, _p(pool_size), _p(ws), nbytes, _s()), 'nnr_pool_archive_ranks',
                unsupported=_ARCHIVES_UNSUPPORTED % archives + 'so are 2^31 user rows, news rows or targets and more')
        return ahead, t_score, pool_size
    L.check(L.lib().nnr_pool_ranks(_p(user), n_user, ldu, _p(reps), n_reps, ldr, D, _p(_u8(valid)), _p(exclude), E, ld_ex, _p(t_off),
                                   _p(t_news) if T else None, T, _p(ahead) if T else None, _p(t_score) if T else None, _p(pool_size), _p(ws),
                                   nbytes, _s()), 'nnr_pool_ranks', unsupported='2^31 user rows, news rows or targets and more are unsupported')
    return ahead, t_score, pool_size


def cne_pair_triples(hist, cand, tlen, clen, batch_size, first=0, count=None, check=True):
    """The pairing plan of the rank-pairing CNE encoders for the reference batches of the samples first .. first + count - 1
    (nnr_cne_pair_triples, include/nnr_hip.h): hist int32 [n, H], cand int32 [n], tlen / clen int32 [news] ->
    (pc_hist, pt_hist) int32 [count, H] and (pc_cand, pt_cand) int32 [count]: the news whose content memory gates the title, and whose
    title memory gates the content, of every history slot / candidate.  The range is whole reference batches: `first` is a multiple of batch_size
    and the range ends at a batch boundary or with the split.  check=True reads the
    ranges of the ids and lengths back (one sync) and raises before the launch; a caller that plans many windows checks once."""
    i32 = torch.int32
    if hist.dim() != 2 or cand.dim() != 1 or cand.numel() != hist.shape[0] or tlen.dim() != 1 or clen.numel() != tlen.numel():
        raise L.NnrHipError('cne_pair_triples: hist [n, H], cand [n] and two length tables of one size')
    if any(x.dtype != i32 or not x.is_contiguous() for x in (hist, cand, tlen, clen)):
        raise L.NnrHipError('cne_pair_triples: hist, cand, tlen and clen must be contiguous int32 tensors')
    n, H = hist.shape
    count = n - first if count is None else count
    if batch_size < 1 or H < 1 or count < 1 or first < 0 or first % batch_size or first + count > n or (first + count < n and count % batch_size):
        raise L.NnrHipError('cne_pair_triples: samples %d .. %d of %d in batches of %d (the range starts and ends at a batch boundary inside the split)'
                            % (first, first + count - 1, n, batch_size))
    if check:
        _p(hist), _p(cand), _p(tlen), _p(clen)
        lo_h, hi_h, lo_c, hi_c, lo_t, hi_t, lo_l, hi_l = torch.stack(torch.aminmax(hist) + torch.aminmax(cand) + torch.aminmax(tlen)
                                                                       + torch.aminmax(clen)).tolist()
        if min(lo_h, lo_c) < 0 or max(hi_h, hi_c) >= tlen.numel():
            raise L.NnrHipError('cne_pair_triples: news ids %d..%d for %d news' % (min(lo_h, lo_c), max(hi_h, hi_c), tlen.numel()))
        if min(lo_t, lo_l) < 0 or max(hi_t, hi_l) > 255:
            raise L.NnrHipError('cne_pair_triples: lengths %d..%d outside the 256 bins of the counting sort' % (min(lo_t, lo_l), max(hi_t, hi_l)))
    out = torch.empty(2 * count * (H + 1), device=hist.device, dtype=i32)
    tmp = torch.empty(2 * count * (H + 1), device=hist.device, dtype=i32)
    pc_h, pt_h = out[:count * H].view(count, H), out[count * H:2 * count * H].view(count, H)
    pc_c, pt_c = out[2 * count * H:2 * count * H + count], out[2 * count * H + count:]
    L.check(L.lib().nnr_cne_pair_triples(_p(hist), _p(cand), _p(tlen), _p(clen), n, H, tlen.numel(), batch_size, first, count, _p(pc_h), _p(pt_h),
                                         _p(pc_c), _p(pt_c), _p(tmp), _s()), 'nnr_cne_pair_triples',
            unsupported='batch_size * H or the number of calls beyond 2^31')
    return pc_h, pt_h, pc_c, pt_c


def nls_loss(logits, B, N, loss, dlogits):
    L.check(L.lib().nnr_nls_loss(_p(logits), B, N, _p(loss), _p(dlogits), _s()), 'nnr_nls_loss')


def logits_bwd(dlogits, user, cand, B, N, D, duser, dcand, accumulate=False):
    L.check(L.lib().nnr_logits_bwd(_p(dlogits), _p(user), _p(cand), B, N, D, _p(duser), _p(dcand), accumulate, _s()), 'nnr_logits_bwd')


def sumsq(g, out):
    """out[0] = sum g^2 (stored; fixed-order sum)."""
    with _hbm_span('sumsq', 4.0, g.numel()):
        return _sumsq(g, out)


def _sumsq(g, out):
    L.check(L.lib().nnr_sumsq(_p(g), g.numel(), _p(out), _s()), 'nnr_sumsq')


def sumsq_part(g, out, add_in=None, slot=0):
    """out[0] = sum g^2 (+ add_in[0]) over one span of the flat gradient (fixed-order sum; `slot`: scratch set, one per concurrent stream)."""
    with _hbm_span('sumsq', 4.0, g.numel()):
        L.check(L.lib().nnr_sumsq_part(_p(g), g.numel(), _p(out), _p(add_in), slot, _s()), 'nnr_sumsq_part')


def fusion_rows_fwd(cat_table, sub_table, cat0, sub0, cat1, sub1, out_view, ldo, p, seed_cat, seed_sub):
    """feature_fusion's category / subCategory rows of one encoder call (cat1 = sub1 = None) or of the union of two calls."""
    n0, n1 = cat0.numel(), (cat1.numel() if cat1 is not None else 0)
    L.check(L.lib().nnr_fusion_rows_fwd(_p(cat_table), _p(sub_table), _p(cat0), _p(sub0), n0, _p(cat1), _p(sub1), n1, cat_table.shape[1],
                                        sub_table.shape[1], _p(out_view), ldo, p, seed_cat, seed_sub, _s()), 'nnr_fusion_rows_fwd')


def fusion_rows_bwd(cat0, sub0, cat1, sub1, cd, sd, dout_view, lddo, dcat_table, dsub_table, p, seed_cat, seed_sub):
    n0, n1 = cat0.numel(), (cat1.numel() if cat1 is not None else 0)
    if cd <= 128 and sd <= 128:                   # reproducible form (slot rows + fixed-order sum); wider tables: f32 atomics
        L.check(L.lib().nnr_fusion_rows_bwd_det(_p(cat0), _p(sub0), n0, _p(cat1), _p(sub1), n1, cd, sd, dcat_table.shape[0], dsub_table.shape[0],
                                                _p(dout_view), lddo, _p(dcat_table), _p(dsub_table), p, seed_cat, seed_sub, _s()),
                                                'nnr_fusion_rows_bwd_det')
        return
    L.check(L.lib().nnr_fusion_rows_bwd(_p(cat0), _p(sub0), n0, _p(cat1), _p(sub1), n1, cd, sd, _p(dout_view), lddo, _p(dcat_table), _p(dsub_table),
                                        p, seed_cat, seed_sub, _s()), 'nnr_fusion_rows_bwd')


def click_loss(user, cand, B, N, D, logits, loss, dlogits, duser, dcand, terms_ws):
    """logits, loss, d loss / d logits, d user, d cand in one launch (model.py:126-127, trainer.py:64-66)."""
    L.check(L.lib().nnr_click_loss(_p(user), _p(cand), B, N, D, _p(logits), _p(loss), _p(dlogits), _p(duser), _p(dcand), _p(terms_ws), _s()),
            'nnr_click_loss')


def clip_adam(p, g, m, v, sumsq_buf, grad_scale, clip, lr, beta1, beta2, eps, wd, step):
    with _hbm_span('clip_adam', 7 * 4.0, p.numel()):                              # p, g, m, v read; p, m, v written
        return _clip_adam(p, g, m, v, sumsq_buf, grad_scale, clip, lr, beta1, beta2, eps, wd, step)


def _clip_adam(p, g, m, v, sumsq_buf, grad_scale, clip, lr, beta1, beta2, eps, wd, step):
    L.check(L.lib().nnr_clip_adam(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(sumsq_buf), grad_scale, clip, lr, beta1, beta2, eps, wd, step, _s()),
                                  'nnr_clip_adam')


def mhsa_fwd(qkv, mask, n, Lq, heads, dh, out, prob, p=0.0, seed=0):
    """p > 0: the dropout that follows the attention is applied in the output stage (== ops.dropout(out, p, seed))."""
    if mask is not None and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    with _mhsa_span('mhsa_fwd', n, Lq, heads, dh, 4.0, 4.0):          # S = Q K^T and O = P V: 4 L^2 d FLOP per head; Q, K, V read, O written
        return _mhsa_fwd(qkv, mask, n, Lq, heads, dh, out, prob, p, seed)


def _mhsa_span(family, n, Lq, heads, dh, flop_units, arrays):
    if not _prof.active():
        return _NOSPAN

    def flops(vals=None):
        return flop_units * Lq * Lq * dh * heads * n

    def nbytes(vals=None):
        return arrays * 4.0 * n * Lq * heads * dh
    flops.dyn = []
    flops.bytes_fn = nbytes
    flops.tag = 'n%d L%d h%d d%d' % (n, Lq, heads, dh)
    return _prof.span(family, flops)


def _mhsa_fwd(qkv, mask, n, Lq, heads, dh, out, prob, p, seed):
    L.check(L.lib().nnr_mhsa_fwd(_p(qkv), _p(mask), n, Lq, heads, dh, 1.0 / math.sqrt(dh), _p(out), _p(prob), p, seed, _s()), 'nnr_mhsa_fwd')


def mhsa_bwd(qkv, mask, prob, dout, n, Lq, heads, dh, dqkv, p=0.0, seed=0):
    if mask is not None and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    # P recomputed (2), dP = dO V^T (2), dV = P^T dO (2), dQ = dS K (2), dK = dS^T Q (2): 10 L^2 d FLOP per head; Q, K, V, dO read, dQ, dK, dV written
    with _mhsa_span('mhsa_bwd', n, Lq, heads, dh, 10.0, 7.0):
        return _mhsa_bwd(qkv, mask, prob, dout, n, Lq, heads, dh, dqkv, p, seed)


def _mhsa_bwd(qkv, mask, prob, dout, n, Lq, heads, dh, dqkv, p, seed):
    L.check(L.lib().nnr_mhsa_bwd(_p(qkv), _p(mask), _p(prob), _p(dout), n, Lq, heads, dh, 1.0 / math.sqrt(dh), _p(dqkv), p, seed, _s()),
                                 'nnr_mhsa_bwd')


def mask_cover(mask):
    """cover[i][t] = 1 for t <= the last valid position of row i, all ones for a row without a valid position (csrc/seq_plan.hip)."""
    m8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    assert m8.is_contiguous() and m8.dim() == 2
    out = torch.empty_like(m8)
    L.check(L.lib().nnr_mask_cover(_p(m8), m8.shape[0], m8.shape[1], _p(out), _s()), 'nnr_mask_cover')
    return out


def seq_rowmap(plan):
    """[n * L] int32: packed row of position t of sequence i (plan.off[t] + plan.rank[i]) or -1 beyond the sequence's length."""
    out = torch.empty(plan.n * plan.L, device=plan.off.device, dtype=torch.int32)
    L.check(L.lib().nnr_seq_rowmap(_p(plan.off), _p(plan.rank), _p(plan.len), plan.n, plan.L, _p(out), _s()), 'nnr_seq_rowmap')
    return out


def _mhsa_span_packed(family, plan, heads, dh, flop_units, arrays):
    """MFMA work as the dense form (the kernel still multiplies 32 x 32 tiles); HBM bytes over the LIVE rows only."""
    if not _prof.active():
        return _NOSPAN
    n, Lq = plan.n, plan.L

    def flops(vals=None):
        return flop_units * Lq * Lq * dh * heads * n

    def nbytes(vals=None, total=plan.total):
        rows = min(n * Lq, int(vals[total.data_ptr()]) if vals is not None else int(total.reshape(-1)[0].item()))
        return arrays * 4.0 * rows * heads * dh
    flops.dyn = [plan.total]
    flops.bytes_fn = nbytes
    flops.tag = 'n%d L%d h%d d%d packed' % (n, Lq, heads, dh)
    return _prof.span(family, flops)


def mhsa_fwd_packed(qkv, mask, rowmap, plan, heads, dh, out, p=0.0, seed=0):
    if mask is not None and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    with _mhsa_span_packed('mhsa_fwd', plan, heads, dh, 4.0, 4.0):
        L.check(L.lib().nnr_mhsa_fwd_packed(_p(qkv), _p(mask), _p(rowmap), plan.n, plan.L, heads, dh, 1.0 / math.sqrt(dh), _p(out), p, seed, _s()),
                                            'nnr_mhsa_fwd_packed')


def mhsa_bwd_packed(qkv, mask, rowmap, plan, dout, heads, dh, dqkv, p=0.0, seed=0):
    if mask is not None and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    with _mhsa_span_packed('mhsa_bwd', plan, heads, dh, 10.0, 7.0):
        L.check(L.lib().nnr_mhsa_bwd_packed(_p(qkv), _p(mask), _p(rowmap), _p(dout), plan.n, plan.L, heads, dh, 1.0 / math.sqrt(dh), _p(dqkv), p,
                                            seed, _s()), 'nnr_mhsa_bwd_packed')


def mhsa_pair_map(plan, mask):
    """(vrowmap [n, 32] int32, vmask [n, 32] uint8) of the paired attention core over `plan` (a packed call with L = 32) and the ORIGINAL key mask."""
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    vrow = torch.empty((plan.n, plan.L), device=plan.off.device, dtype=torch.int32)
    vmask = torch.empty((plan.n, plan.L), device=plan.off.device, dtype=torch.uint8)
    L.check(L.lib().nnr_mhsa_pair_map(_p(plan.off), _p(plan.slen), _p(plan.order), _p(mask.contiguous()), plan.n, plan.L, _p(vrow), _p(vmask), _s()),
            'nnr_mhsa_pair_map')
    return vrow, vmask


def mhsa_fwd_paired(qkv, pair, plan, heads, dh, out, p=0.0, seed=0):
    vrow, vmask = pair
    with _mhsa_span_packed('mhsa_fwd', plan, heads, dh, 4.0, 4.0):
        L.check(L.lib().nnr_mhsa_fwd_paired(_p(qkv), _p(vmask), _p(vrow), _p(plan.off), plan.n, heads, dh, 1.0 / math.sqrt(dh), _p(out), p, seed,
                                            _s()), 'nnr_mhsa_fwd_paired')


def mhsa_bwd_paired(qkv, pair, plan, dout, heads, dh, dqkv, p=0.0, seed=0):
    vrow, vmask = pair
    with _mhsa_span_packed('mhsa_bwd', plan, heads, dh, 10.0, 7.0):
        L.check(L.lib().nnr_mhsa_bwd_paired(_p(qkv), _p(vmask), _p(vrow), _p(plan.off), _p(dout), plan.n, heads, dh, 1.0 / math.sqrt(dh), _p(dqkv), p,
                                            seed, _s()), 'nnr_mhsa_bwd_paired')


def mhsa_prob_size(n, Lq, heads):
    nb = 2 if Lq > 32 else 1
    return n * heads * nb * nb * 1024


def embed_gather(table, idx, p, seed, out=None, dyn=None):
    """out[row] = dropout(table[idx[row]]); `dyn`: device int32 holding the live row count (rows beyond it are left untouched)."""
    n, dim = idx.numel(), table.shape[1]
    if out is None:
        out = torch.empty((n, dim), device=table.device, dtype=torch.float32)
    with _hbm_span('embed_gather', 2 * 4.0 * dim + 4.0, n, dyn=dyn):              # a table row read, a row written, an id read
        return _embed_gather(table, idx, p, seed, out, dyn, n, dim)


def _embed_gather(table, idx, p, seed, out, dyn, n, dim):
    L.check(L.lib().nnr_embed_gather(_p(table), _p(idx), n, _p(dyn), dim, _p(out), p, seed, _s()), 'nnr_embed_gather')
    return out


def embed_scatter(dout, idx, dtable, p, seed, dyn=None):
    n, dim = idx.numel(), dtable.shape[1]
    with _hbm_span('embed_scatter', 2 * 4.0 * dim + 4.0, n, dyn=dyn):             # a gradient row read, a table-gradient row added to, an id read
        return _embed_scatter(dout, idx, dtable, p, seed, dyn, n, dim)


def _embed_scatter(dout, idx, dtable, p, seed, dyn, n, dim):
    if dyn is not None:
        L.check(L.lib().nnr_embed_scatter_dyn(_p(dout), _p(idx), n, _p(dyn), dim, _p(dtable), p, seed, _s()), 'nnr_embed_scatter_dyn')
        return
    L.check(L.lib().nnr_embed_scatter(_p(dout), _p(idx), n, dim, _p(dtable), p, seed, _s()), 'nnr_embed_scatter')


def _sort_on_leaf(tok, total, vocab):
    """`tok` (int32 keys; total: device count of the live ones, or None for all) sorted by key on the LEAF stream behind the current stream's
    work (csrc/sort.hip; stable) -> (sorted keys, their positions in `tok`, the event its consumers wait for)."""
    dev, cap = tok.device, tok.numel()
    buf = torch.empty(4 * cap, device=dev, dtype=torch.int32)    # keys_tmp | pos_tmp | keys_sorted | pos_sorted
    temp = torch.empty(max(L.lib().nnr_token_sort_workspace_bytes(cap, vocab), 256), device=dev, dtype=torch.uint8)
    leaf = leaf_stream(dev)
    leaf.wait_stream(torch.cuda.current_stream(dev))              # behind the launch that wrote `tok` / `total`
    with torch.cuda.stream(leaf):
        L.check(L.lib().nnr_token_sort(_p(tok), cap, _p(total), vocab, _p(buf[:cap]), _p(buf[cap:2 * cap]), _p(buf[2 * cap:3 * cap]), _p(buf[3 * cap:]),
                                       _p(temp), temp.numel(), _s()), 'nnr_token_sort')
        event = torch.cuda.Event()
        event.record()
    # a graph that is dropped without a backward pass frees these while the sort may still run: the allocator must wait for the leaf
    # stream before it hands them out again (a few MB, unlike the GB-sized buffers leaf_scope holds by reference instead)
    for t in (tok, buf, temp):
        t.record_stream(leaf)
    return buf[2 * cap:3 * cap], buf[3 * cap:], event


class TokenSort:
    """The live rows of a packed token stream sorted by word id (csrc/sort.hip), issued on the LEAF stream behind the planner: it
    needs nothing but the planned ids, so it runs under the forward pass; the backward's nnr_embed_scatter_sorted waits for `event`."""

    def __init__(self, tok, total, vocab):
        self.cap, self.vocab, self.total = tok.numel(), int(vocab), total
        self.partial = torch.empty(L.lib().nnr_embed_scatter_sorted_workspace_floats(self.cap), device=tok.device, dtype=torch.float32)
        self.keys, self.rows, self.event = _sort_on_leaf(tok, total, self.vocab)


def embed_scatter_sorted(dout, ts, dtable, p, seed):
    """dtable[w] += sum of mask * dout[row] over the rows of word w in list order (reproducible; see TokenSort)."""
    dim = dtable.shape[1]
    torch.cuda.current_stream(dout.device).wait_event(ts.event)
    with _hbm_span('embed_scatter', 2 * 4.0 * dim + 8.0, ts.cap, dyn=ts.total, tag='sorted cap%d' % ts.cap):
        L.check(L.lib().nnr_embed_scatter_sorted(_p(dout), _p(ts.keys), _p(ts.rows), ts.cap, ts.vocab, dim, _p(dtable), p, seed, _p(ts.partial),
                                                 _s()), 'nnr_embed_scatter_sorted')


# ---------------------------------------------------------------------------------------------- bag of words (csrc/bag.hip)
BAG_UNSUPPORTED = 'unsupported size (a stream of more than 128 positions or word_embedding_dim > 320)'


class OccurrencePlan:
    """Occurrence list of one bag forward call for its backward pass: `tok` [cap] (written by the forward launch: word id of a live
    position, -1 elsewhere) sorted by word id on the LEAF stream behind the forward launch (csrc/sort.hip; stable, so a word's
    occurrences keep their order in `tok`), and the workspace of the backward's reduction (csrc/sorted_rows.h).  Nothing is read on the
    host."""

    def __init__(self, cap, ws_floats, vocab, dev):
        self.cap, self.vocab = cap, int(vocab)
        self.tok = torch.empty(max(cap, 1), device=dev, dtype=torch.int32)[:cap]
        self.partial = torch.empty(max(ws_floats, 1), device=dev, dtype=torch.float32)
        self.event = None

    def sort(self):
        self.keys, self.pos, self.event = _sort_on_leaf(self.tok, None, self.vocab)


class BagPlan(OccurrencePlan):
    """The plan of one bag_mean_fwd call: `tok` is [n, La + Lb], so a word's occurrences keep the order news row, stream a, stream b, position."""

    def __init__(self, n, La, Lb, vocab, dev):
        self.n, self.La, self.Lb = n, La, Lb
        cap = n * (La + Lb)
        super().__init__(cap, L.lib().nnr_bag_mean_bwd_ws_floats(cap), vocab, dev)


def bag_mean_fwd(table, ids_a, mask_a, ids_b, mask_b, separate, act, out, ldo, off_a, off_b, count, plan=None, live=None):
    """Masked mean of table rows over the live positions of ids_a [n, La] (+ ids_b [n, Lb], optional); see include/nnr_hip.h.  Masks are
    bool / uint8 [n, L], written in place (column 0) when `separate`.  plan: a BagPlan whose `tok` the launch fills.  live (profiling
    only): live positions of the call, for the byte count.  Returns 0; every failure raises (sizes beyond the limits: BAG_UNSUPPORTED)."""
    n, La = ids_a.shape
    Lb = ids_b.shape[1] if ids_b is not None else 0
    V, E = table.shape
    # per news: ids + mask bytes read, one or two output rows + counts written (+ the occurrence keys); per live position one table row
    per_row = 5.0 * (La + Lb) + 4.0 * E * (2 if separate and ids_b is not None else 1) + 8.0 + (4.0 * (La + Lb) if plan is not None else 0.0)
    with _hbm_span('bag_mean_fwd', per_row, n, fixed=4.0 * E * (live if live is not None else n * (La + Lb))):
        rc = L.lib().nnr_bag_mean_fwd(_p(table), V, E, _p(ids_a), _p(_u8(mask_a)), La, _p(ids_b), _p(_u8(mask_b)), Lb, n, int(bool(separate)), act,
                                      _p(out), ldo, off_a, off_b, _p(count), _p(plan.tok) if plan is not None else None, _s())
    L.check(rc, 'nnr_bag_mean_fwd', BAG_UNSUPPORTED)
    return 0


def bag_mean_bwd(dout, lddo, out, ldo, off_a, off_b, count, plan, separate, act, dtable, live=None):
    """dtable[w] += sum over w's live occurrences of g[r] / count (reproducible, no float atomics); waits for the plan's sort."""
    E = dtable.shape[1]
    torch.cuda.current_stream(dout.device).wait_event(plan.event)
    # per sorted entry a key + a position; per live occurrence a gradient row (and an output row behind the sigmoid) read from the n
    # rows of the call, and -- counted once per occurrence, an upper bound -- a table-gradient row read and written
    rows = 1 if act == ACT_NONE else 2
    with _hbm_span('bag_mean_bwd', 8.0, plan.cap, fixed=4.0 * E * (rows * plan.n + 2.0 * (live if live is not None else plan.cap))):
        L.check(L.lib().nnr_bag_mean_bwd(_p(dout), lddo, _p(out), ldo, off_a, off_b, _p(count), _p(plan.keys), _p(plan.pos), plan.cap, plan.La,
                                         plan.Lb, plan.n, plan.vocab, E, int(bool(separate)), act, _p(dtable), _p(plan.partial), _s()),
                'nnr_bag_mean_bwd')


def row_dist_fwd(a, b, coef, dist, aux, lda=None, ldb=None):
    """dist[r] = ||a[r] - b[r]||_2, aux[r] = coef * dist[r] for a, b [n, D] (leading dimensions allowed)."""
    n, D = a.shape
    with _hbm_span('row_dist_fwd', 2 * 4.0 * D + 8.0, n):
        L.check(L.lib().nnr_row_dist_fwd(_p(a), a.stride(0) if lda is None else lda, _p(b), b.stride(0) if ldb is None else ldb, n, D, coef,
                                         _p(dist), _p(aux), _s()), 'nnr_row_dist_fwd')


def row_dist_bwd(a, b, dist, gup, coef, da, db):
    """da[r] += u, db[r] -= u with u = gup[r] * coef * (a[r] - b[r]) / dist[r] (nothing where dist[r] == 0); gup: device [n]."""
    n, D = a.shape
    with _hbm_span('row_dist_bwd', 6 * 4.0 * D + 8.0, n):
        L.check(L.lib().nnr_row_dist_bwd(_p(a), a.stride(0), _p(b), b.stride(0), _p(dist), _p(gup), n, D, coef, _p(da), da.stride(0), _p(db),
                                         db.stride(0), _s()), 'nnr_row_dist_bwd')


# ---------------------------------------------------------------------------------------------- DSSM (csrc/dssm.hip)
WBAG_MAXE, WBAG_MAXL = 1024, 4096      # nnr_wbag_dims' rule, restated so that a constructor can refuse a size without the library
WBAG_UNSUPPORTED = 'unsupported size (a weighted bag takes 1 <= hidden dim <= 1024 and 1 <= positions per row <= 4096)'


def wbag_supported(E, La, Lb=0):
    """nnr_wbag_dims' rule without a library call."""
    return 1 <= E <= WBAG_MAXE and 1 <= La <= WBAG_MAXL and 0 <= Lb <= WBAG_MAXL


def wbag_dims(E, La, Lb=0):
    """(chunk length, chunks per row of stream a, of stream b) of the weighted bag; sizes beyond the rule raise WBAG_UNSUPPORTED."""
    chunk, ca, cb = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().nnr_wbag_dims(E, La, Lb, C.addressof(chunk), C.addressof(ca), C.addressof(cb)), 'nnr_wbag_dims', WBAG_UNSUPPORTED, counted=False)
    return chunk.value, ca.value, cb.value


def _wstream(s):
    """A weighted-bag stream (ids int32 [R, L], w f32 [R, L], sel int32 [n] or None) -> (ids, w, sel, R, n, L); None: no stream."""
    if s is None:
        return None, None, None, 0, 0, 0
    ids, w, sel = s
    R, Lx = w.shape
    assert ids.shape == w.shape and ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.is_contiguous() and w.is_contiguous()
    assert sel is None or (sel.dtype == torch.int32 and sel.is_contiguous())
    return ids, w, sel, R, (sel.numel() if sel is not None else R), Lx


class WbagPlan(OccurrencePlan):
    """The plan of one wbag_fwd call: `tok` is [na * La + nb * Lb], so a word's occurrences keep the order stream a, stream b, row, position."""

    def __init__(self, cap, E, vocab, dev):
        super().__init__(cap, L.lib().nnr_wbag_bwd_ws_floats(cap, E), vocab, dev)


def wbag_fwd(table, sa, sb, p, seed_a, seed_b, out, plan=None):
    """out [na + nb, E] = the weighted bags of both streams (see include/nnr_hip.h); sa / sb: (ids, w, sel) as _wstream takes them, sb may
    be None.  plan: a WbagPlan whose `tok` the launch fills.  Sizes beyond the rule raise WBAG_UNSUPPORTED."""
    V, E = table.shape
    ia, wa, sla, Ra, na, La = _wstream(sa)
    ib, wb, slb, Rb, nb, Lb = _wstream(sb)
    assert out.shape == (na + nb, E) and out.is_contiguous() and table.is_contiguous()
    if not wbag_supported(E, La, Lb):
        raise L.NnrHipError('nnr_wbag_fwd: ' + WBAG_UNSUPPORTED)
    ws = torch.empty(max(L.lib().nnr_wbag_fwd_ws_floats(na, La, nb, Lb, E), 1), device=table.device, dtype=torch.float32)
    L.check(L.lib().nnr_wbag_fwd(_p(table), V, E, _p(ia), _p(wa), _p(sla), Ra, na, La, _p(ib), _p(wb), _p(slb), Rb, nb, Lb, p, seed_a, seed_b,
                                 _p(out), _p(plan.tok) if plan is not None else None, _p(ws), _s()), 'nnr_wbag_fwd', WBAG_UNSUPPORTED)
    return out


def wbag_bwd(dout, sa, sb, p, seed_a, seed_b, plan, dtable):
    """dtable[w] += sum over w's live occurrences of keep * scale * weight * dout[row] (reproducible, no float atomics); waits for the
    plan's sort."""
    V, E = dtable.shape
    _, wa, sla, Ra, na, La = _wstream(sa)
    _, wb, slb, Rb, nb, Lb = _wstream(sb)
    assert dout.shape == (na + nb, E) and dout.is_contiguous() and plan.cap == na * La + nb * Lb
    torch.cuda.current_stream(dout.device).wait_event(plan.event)
    L.check(L.lib().nnr_wbag_bwd(_p(dout), _p(plan.keys), _p(plan.pos), plan.cap, _p(wa), _p(sla), Ra, na, La, _p(wb), _p(slb), Rb, nb, Lb, V, E,
                                 p, seed_a, seed_b, _p(dtable), _p(plan.partial), _s()), 'nnr_wbag_bwd', WBAG_UNSUPPORTED)


def cosine_loss(user, news, B, N, F, logits, loss=None, dlogits=None, duser=None, dnews=None, ws=None):
    """Cosine click head (+ loss and every gradient, when their buffers are given) in one launch; loss .. dnews all None: logits only."""
    L.check(L.lib().nnr_cosine_loss(_p(user), _p(news), B, N, F, _p(logits), _p(loss), _p(dlogits), _p(duser), _p(dnews), _p(ws), _s()),
            'nnr_cosine_loss', 'unsupported size (more than 64 candidates per sample)')


def tanh_drop_bwd(dy, t, dz, p, seed):
    """dz = mask(dy) * (1 - t * t): backward of y = dropout(tanh(z)) given t = tanh(z)."""
    L.check(L.lib().nnr_tanh_drop_bwd(_p(dy), _p(t), _p(dz), dy.numel(), p, seed, _s()), 'nnr_tanh_drop_bwd')


# ---------------------------------------------------------------------------------------------- weight layouts (nnr_permute, csrc/misc.hip)
def _pad4(n):
    return (n + 3) & ~3


# kind -> dims -> (extents n0..n3, source strides, destination strides, source offset, destination shape), strides and offset in floats, the
# destination's unit-stride axis last.  Source: the weight as torch holds it (or, for the *_dw kinds, the gradient of its permuted form).
LAYOUTS = {
    # Conv weight W [C, E, w, J] of the padded-row convolution (KCNN's Conv2d, which the kinds are named after: J = 3; Conv1d [C, E, w]: J = 1):
    # P[c][dt][j][e] | Q[j][e][k][c] = W[c][e][w-1-k][j] | W.grad[c][e][dt][j] += dP[c][dt][j][e]
    'kcnn_p': lambda C_, E, w, J=3: ((C_, w, J, E), (E * w * J, J, 1, w * J), (w * J * E, J * E, E, 1), 0, (C_, J * w * E)),
    'kcnn_q': lambda C_, E, w, J=3: ((J, E, w, C_), (1, w * J, -J, E * w * J), (E * w * C_, w * C_, C_, 1), (w - 1) * J, (J * E, w * C_)),
    'kcnn_dw': lambda C_, E, w, J=3: ((C_, E, w, J), (w * J * E, 1, J * E, E), (E * w * J, w * J, J, 1), 0, (C_, E, w, J)),
    # Conv1d weight W [F, C, w]: P[k][f][c] in rows of ldp >= C floats | W.grad[f][c][k] += dP[k][f][c]
    'hdc_p': lambda F, C_, w, ldp: ((1, w, F, C_), (0, 1, C_ * w, w), (0, F * ldp, ldp, 1), 0, (w, F, ldp)),
    'hdc_dw': lambda F, C_, w, ldp: ((1, F, C_, w), (0, ldp, 1, F * ldp), (0, C_ * w, w, 1), 0, (F, C_, w)),
    # Conv3d weight W [Cout, Cin, K^3]: [ci][t][f] in rows of Cout rounded up to 4 | [f][t][ci] in rows of Cin rounded up to 4
    'c3_p': lambda Co, Ci, K: ((1, Ci, K ** 3, Co), (0, K ** 3, 1, Ci * K ** 3), (0, K ** 3 * _pad4(Co), _pad4(Co), 1), 0, (Ci, K ** 3, _pad4(Co))),
    'c3_q': lambda Co, Ci, K: ((1, Co, K ** 3, Ci), (0, Ci * K ** 3, 1, K ** 3), (0, K ** 3 * _pad4(Ci), _pad4(Ci), 1), 0, (Co, K ** 3, _pad4(Ci))),
}


def permute(src, out, kind, dims, accumulate=False):
    """out (+)= src in the layout LAYOUTS[kind](*dims), both contiguous; every address is checked against the two sizes here."""
    n, si, so, off, _ = LAYOUTS[kind](*dims)
    assert src.is_contiguous() and out.is_contiguous()
    for t, strides, base in ((src, si, off), (out, so, 0)):
        lo = base + sum((m - 1) * st for m, st in zip(n, strides) if st < 0)
        hi = base + sum((m - 1) * st for m, st in zip(n, strides) if st > 0)
        assert 0 <= lo and hi < t.numel(), (kind, dims, tuple(t.shape))
    L.check(L.lib().nnr_permute(_p(src) + 4 * off, _p(out), *n, *si, *so, int(accumulate), _s()), 'nnr_permute')


def _permuted_weight(kind, weight, dims):
    """`weight` in the layout `kind`, an entry of the derived-weight cache.  Elements of the layout that the permute does not reach (the pad
    columns of a row) are zeroed once, when the entry's buffer is made: nothing else ever writes it."""
    n, _, _, _, shape = LAYOUTS[kind](*dims)
    padded = math.prod(shape) != math.prod(n)
    e = _derived(kind, weight, dims, lambda: (torch.zeros if padded else torch.empty)(shape, device=weight.device, dtype=torch.float32), False)
    _serve(e, (weight,), lambda: permute(weight, e.out, kind, dims))
    return e.out


# ---------------------------------------------------------------------------------------------- KCNN / DKN (csrc/kcnn.hip)
KCNN_UNSUPPORTED = 'unsupported size (max_title_length + cnn_window_size - 1 > 255, cnn_window_size > 8 or > max_title_length, or word_embedding_dim > 1024)'


def kcnn_image_fwd(table, text, pre1, pre2, n, Lx, w, Xp):
    """Xp [n, Lx + w - 1, 3, E]: zero halo rows, [word row | tanh(pre1) | tanh(pre2)] per title position (include/nnr_hip.h)."""
    V, E = table.shape
    # per padded row 3 E floats written; per title position an id, a table row and two pre-activation rows read
    with _hbm_span('kcnn_image_fwd', 3 * 4.0 * E, n * (Lx + w - 1), fixed=(3 * 4.0 * E + 4.0) * n * Lx):
        L.check(L.lib().nnr_kcnn_image_fwd(_p(table), V, _p(text), _p(pre1), _p(pre2), n, Lx, E, w, _p(Xp), _s()), 'nnr_kcnn_image_fwd', KCNN_UNSUPPORTED)


def kcnn_image_bwd(dXp, Xp, n, Lx, E, w, dx0, dpre1, dpre2):
    """dx0 / dpre1 / dpre2 [n * Lx, E] from the padded gradient image (the tanh derivative from the forward image's channels 1 and 2)."""
    with _hbm_span('kcnn_image_bwd', (3 + 2 + 3) * 4.0 * E, n * Lx):
        L.check(L.lib().nnr_kcnn_image_bwd(_p(dXp), _p(Xp), n, Lx, E, w, _p(dx0), _p(dpre1), _p(dpre2), _s()), 'nnr_kcnn_image_bwd', KCNN_UNSUPPORTED)


def window_max_fwd(z, ldz, bias, n, C, Lx, w, out, arg):
    """out [n, C] = relu-then-max over the first Lx - w + 1 positions of z + bias, arg [n, C] uint8 (255: no positive maximum)."""
    with _hbm_span('window_max_fwd', 4.0 * C * (Lx - w + 1) + 5.0 * C, n):
        L.check(L.lib().nnr_window_max_fwd(_p(z), ldz, _p(bias), n, C, Lx, w, _p(out), _p(arg), _s()), 'nnr_window_max_fwd', KCNN_UNSUPPORTED)


def window_max_bwd(g, arg, n, C, Lx, w, lead, dz, db):
    """dz [lead + n * (Lx + w - 1), C] written densely, db [C] written (fixed-order column sum of the gradients that reached a position)."""
    ws = torch.empty(max(1, L.lib().nnr_window_max_bwd_ws_floats(n, C)), device=g.device, dtype=torch.float32)
    tape_keep(ws)
    with _hbm_span('window_max_bwd', 4.0 * C * (Lx + w - 1) + 5.0 * C, n):
        L.check(L.lib().nnr_window_max_bwd(_p(g), _p(arg), n, C, Lx, w, lead, _p(dz), _p(db), _p(ws), _s()), 'nnr_window_max_bwd', KCNN_UNSUPPORTED)


def rowconv_dims(weight):
    return tuple(weight.shape) if weight.dim() == 4 else tuple(weight.shape) + (1,)          # (C, E, w, J); a Conv1d weight [C, E, w]: J = 1


def rowconv_weight(weight, mode):
    """P [C, J w E] (mode 0) or Q [J E, w C] (mode 1) of the Conv2d weight [C, E, w, J] or the Conv1d weight [C, E, w] (J = 1): the B operand
    of the padded-row convolution product or of its data gradient, an entry of the derived-weight cache (permuted once per parameter
    version, by the first of the two encoder calls that asks; its bf16x3 images follow it)."""
    _, E, w, _ = dims = rowconv_dims(weight)
    if weight.dim() == 4 and (w > 8 or E > 1024):
        raise L.NnrHipError('rowconv_weight: %s' % KCNN_UNSUPPORTED)
    if weight.dim() == 3 and (w > 8 or w % 2 == 0):
        raise L.NnrHipError('rowconv_weight: %s' % CONV1D_UNSUPPORTED)
    return _permuted_weight('kcnn_q' if mode else 'kcnn_p', weight, dims)


# ---------------------------------------------------------------------------------------------- NAML view attention (csrc/naml.hip)
VIEW_POOL_UNSUPPORTED = 'unsupported size (a non-positive dimension, or text views outside 1..2)'


def view_pool_fwd(texts, scores, rowsA, scoreA, idsA, rowsB, scoreB, idsB, alpha, out):
    """out [n, C] = sum over the views of softmax_v(score_v) * row_v; alpha [n, V] (include/nnr_hip.h).  texts / scores: 1 or 2 text views."""
    Vt, (n, Cn) = len(texts), out.shape
    t1, s1 = (texts[1], scores[1]) if Vt == 2 else (None, None)
    # per news: V rows read (the table rows mostly from cache), one row + V weights written, V scores + 2 ids read
    with _hbm_span('view_pool_fwd', 4.0 * Cn * (Vt + 3) + 8.0 * (Vt + 2) + 8.0, n):
        L.check(L.lib().nnr_view_pool_fwd(_p(texts[0]), _p(scores[0]), _p(t1), _p(s1), Vt, _p(rowsA), _p(scoreA), _p(idsA), rowsA.shape[0],
                                          _p(rowsB), _p(scoreB), _p(idsB), rowsB.shape[0], n, Cn, _p(alpha), _p(out), _s()),
                'nnr_view_pool_fwd', VIEW_POOL_UNSUPPORTED)


def view_pool_bwd(dout, texts, rowsA, idsA, rowsB, idsB, alpha, dtexts, dtscores, drowsA, dscoreA, drowsB, dscoreB):
    """The eight gradients of view_pool_fwd, all written (include/nnr_hip.h)."""
    Vt, (n, Cn) = len(texts), dout.shape
    t1, d1, ds1 = (texts[1], dtexts[1], dtscores[1]) if Vt == 2 else (None, None, None)
    ws = torch.empty(2 * n, device=dout.device, dtype=torch.float32)
    # per news: dout read twice (per news, per table view), V rows read, Vt rows written; per table row one row written
    with _hbm_span('view_pool_bwd', 4.0 * Cn * (2 * Vt + 5) + 4.0 * (3 * Vt + 10), n, fixed=4.0 * (Cn + 1) * (rowsA.shape[0] + rowsB.shape[0])):
        L.check(L.lib().nnr_view_pool_bwd(_p(dout), _p(texts[0]), _p(t1), Vt, _p(rowsA), _p(idsA), rowsA.shape[0],
                                          _p(rowsB), _p(idsB), rowsB.shape[0], _p(alpha), n, Cn, _p(dtexts[0]),
                                          _p(dtscores[0]), _p(d1), _p(ds1), _p(drowsA), _p(dscoreA), _p(drowsB), _p(dscoreB), _p(ws), _s()),
                'nnr_view_pool_bwd', VIEW_POOL_UNSUPPORTED)


CONV1D_UNSUPPORTED = 'unsupported size (a non-positive dimension, an even cnn_window_size, or cnn_window_size > 8)'
_C1_ROWMAP = {}


def conv1d_image_fwd(table, text, n, Lx, k, p, seed, Xp):
    """Xp [n, Lx + k - 1, E]: zero halo rows and dropout(table[text]) rows, the mask keyed on the compact rows (include/nnr_hip.h)."""
    V, E = table.shape
    with _hbm_span('conv1d_image_fwd', 4.0 * E, n * (Lx + k - 1), fixed=(4.0 * E + 4.0) * n * Lx):
        L.check(L.lib().nnr_conv1d_image_fwd(_p(table), V, _p(text), n, Lx, E, k, p, seed, _p(Xp), _s()), 'nnr_conv1d_image_fwd', CONV1D_UNSUPPORTED)


def conv1d_dz_pad(dy, y, n, Lx, k, dz):
    """dz [(k - 1) + n (Lx + k - 1), C] written densely: relu backward of the compact dy at the live rows, zero elsewhere."""
    Cn = dy.shape[1]
    with _hbm_span('conv1d_dz_pad', 4.0 * Cn, k - 1 + n * (Lx + k - 1), fixed=8.0 * Cn * n * Lx):
        L.check(L.lib().nnr_conv1d_dz_pad(_p(dy), _p(y), n, Lx, Cn, k, _p(dz), _s()), 'nnr_conv1d_dz_pad', CONV1D_UNSUPPORTED)


def conv1d_image_bwd(dXp, n, Lx, k, p, seed, dx):
    """dx [n Lx, E] = keep-mask * the word rows of dXp [n (Lx + k - 1), E]."""
    E = dx.shape[1]
    with _hbm_span('conv1d_image_bwd', 8.0 * E, n * Lx):
        L.check(L.lib().nnr_conv1d_image_bwd(_p(dXp), n, Lx, E, k, p, seed, _p(dx), _s()), 'nnr_conv1d_image_bwd', CONV1D_UNSUPPORTED)


def conv1d_rowmap(n, Lx, k, dev):
    """int32 [n Lp - (k - 1)]: the compact row i Lx + t of image row i Lp + t, -1 for the rows t >= Lx that straddle two news (the
    product's epilogue drops them); None for k == 1 (no junk rows).  Depends on the shape alone: kept per (n, Lx, k, device)."""
    if k == 1:
        return None
    key = (n, Lx, k, dev.type, dev.index)
    m = _C1_ROWMAP.get(key)
    if m is None:
        if len(_C1_ROWMAP) >= 16:
            _C1_ROWMAP.clear()
        Lp = Lx + k - 1
        t = torch.arange(Lp, device=dev, dtype=torch.int32)[None, :]
        base = (torch.arange(n, device=dev, dtype=torch.int32) * Lx)[:, None]
        m = torch.where(t < Lx, base + t, torch.full_like(base + t, -1)).reshape(-1)[:n * Lp - (k - 1)].contiguous()
        _C1_ROWMAP[key] = m
    tape_keep(m)
    return m


# ---------------------------------------------------------------------------------------------- HDC / FIM (csrc/hdc.hip, csrc/fim.hip)
FIM_UNSUPPORTED = ('unsupported size (conv3D kernel size > 4, maxpooling3D_size > 4 or > maxpooling3D_stride, an axis left without a pool cell, '
                   'or weights + one row of pool cells beyond 160 KB of LDS)')


def hdc_seq_fwd(word, cat_t, sub_t, text, cat, sub, n, Lx, pad, d0, d0p, tok_w, tok_c, tok_s):
    """d0 [n, Lx + 2, E] and its halo-padded copy d0p [n, Lx + 2 + 2 pad, E] from the three tables; the three occurrence lists (include/nnr_hip.h)."""
    E = word.shape[1]
    # per padded row E floats written; per live row a table row read, a compact row written, an id read and three list entries written
    with _hbm_span('hdc_seq_fwd', 4.0 * E, n * (Lx + 2 + 2 * pad), fixed=(2 * 4.0 * E + 16.0) * n * (Lx + 2)):
        L.check(L.lib().nnr_hdc_seq_fwd(_p(word), word.shape[0], _p(cat_t), cat_t.shape[0], _p(sub_t), sub_t.shape[0], _p(text), _p(cat), _p(sub),
                                        n, Lx, E, pad, _p(d0), _p(d0p), _p(tok_w), _p(tok_c), _p(tok_s), _s()), 'nnr_hdc_seq_fwd')


def hdc_ln_relu_fwd(z, z_rows, gamma, beta, n, S, F, eps, y, yp, pad, stats):
    """y [n, S, F] = relu(LayerNorm([F, S])(z rows [0, S) of every news)); yp (optional): the same with `pad` zero halo rows per side."""
    with _hbm_span('hdc_ln_relu_fwd', 4.0 * F * (S + S + (S + 2 * pad if yp is not None else 0)) + 8.0, n, fixed=8.0 * F * S):
        L.check(L.lib().nnr_hdc_ln_relu_fwd(_p(z), z_rows, _p(gamma), _p(beta), n, S, F, eps, _p(y), _p(yp), pad, _p(stats), _s()), 'nnr_hdc_ln_relu_fwd')


def hdc_ln_relu_bwd(dy, y, z, z_rows, stats, gamma, n, S, F, dgamma, dbeta):
    """In place: z becomes the gradient of the LayerNorm input (rows [S, z_rows) of every news zero); dgamma / dbeta [F, S] accumulate."""
    ws = torch.empty(max(1, L.lib().nnr_hdc_ln_bwd_ws_floats(n, S, F)), device=dy.device, dtype=torch.float32)
    tape_keep(ws)
    with _hbm_span('hdc_ln_relu_bwd', 4.0 * F * (2 * 3 * S + z_rows), n, fixed=16.0 * F * S):
        L.check(L.lib().nnr_hdc_ln_relu_bwd(_p(dy), _p(y), _p(z), z_rows, _p(stats), _p(gamma), n, S, F, _p(dgamma), _p(dbeta), _p(ws), _s()),
                'nnr_hdc_ln_relu_bwd')


def hdc_unpad_add(a, bp, n, S, pad, C_, out):
    """out [n, S, C] = a (compact, may be None) + the live rows of bp [n, S + 2 pad, C]."""
    with _hbm_span('hdc_unpad_add', 4.0 * C_ * S * (3 if a is not None else 2), n):
        L.check(L.lib().nnr_hdc_unpad_add(_p(a), _p(bp), n, S, pad, C_, _p(out), _s()), 'nnr_hdc_unpad_add')


def hdc_weight(weight):
    """P [w, F, C] of a Conv1d weight [F, C, w]: tap k's [F, C] matrix is the B operand of the k-th accumulating product (an entry of the
    derived-weight cache: permuted once per parameter version)."""
    F, C_, w = weight.shape
    return _permuted_weight('hdc_p', weight, (F, C_, w, C_))


def match_images_fwd(cand, hist, B, N, H, S, alpha, plane):
    """One level's matching images (userEncoders.py:252-253): plane [B][N S][H S] = alpha cand[b] . hist[b]^T for cand [B N, S, C] and hist
    [B H, S, C] -- one batched product, written in the layout the first convolution layer reads through its strides."""
    C_ = cand.shape[2]
    gemm(cand, hist, plane, M=N * S, N=H * S, K=C_, lda=C_, ldb=C_, ldc=H * S, alpha=alpha, batch=B, strideA=N * S * C_, strideB=H * S * C_,
         strideC=N * S * H * S)


def match_images_bwd(dplane, cand, hist, B, N, H, S, alpha, dcand, dhist):
    """dcand [B N, S, C] = alpha dplane[b] . hist[b], dhist [B H, S, C] = alpha dplane[b]^T . cand[b] (both written)."""
    C_ = cand.shape[2]
    gemm(dplane, hist, dcand, M=N * S, N=C_, K=H * S, lda=H * S, ldb=C_, ldc=C_, trans_b=True, alpha=alpha, batch=B, strideA=N * S * H * S,
         strideB=H * S * C_, strideC=N * S * C_)
    gemm(dplane, cand, dhist, M=H * S, N=C_, K=N * S, lda=H * S, ldb=C_, ldc=C_, trans_a=True, trans_b=True, alpha=alpha, batch=B,
         strideA=N * S * H * S, strideB=N * S * C_, strideC=H * S * C_)


def conv3d_pool_plan(Cin, D, H, W, Cout, K, P, St):
    """Host mirror of the library's shape rules (csrc/fim.hip:c3_shape), for constructors that run without a device: (PD, PH, PW), or
    None where nnr_conv3d_pool_dims returns NNR_ERR_UNSUPPORTED (tests/test_hip_fim_gpu.py compares the two)."""
    if not (1 <= K <= 4 and 1 <= P <= 4 and St >= P):
        return None
    pooled = lambda n: 0 if n - K + 1 < P else (n - K + 1 - P) // St + 1
    PD, PH, PW = pooled(D), pooled(H), pooled(W)
    if min(PD, PH, PW) <= 0:
        return None
    DD, Cp = P + K - 1, (Cout + 3) & ~3
    WW = (PW - 1) * St + DD

    def lds(phb):
        xs = (Cin * DD * ((phb - 1) * St + DD) * WW + 3) & ~3
        return 4 * (xs + Cin * K ** 3 * Cp + phb * PW * P ** 3 * Cp)
    phb = 1
    while phb < PH and phb * PW * P * P * (Cp // 4) < 256 and lds(phb + 1) <= 64 * 1024:
        phb += 1
    return (PD, PH, PW) if lds(phb) <= 160 * 1024 else None


def conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St):
    """(PD, PH, PW) of the fused layer, or NnrHipError('... unsupported size ...')."""
    out = [C.c_int(0) for _ in range(3)]
    L.check(L.lib().nnr_conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St, *[C.addressof(o) for o in out]), 'nnr_conv3d_pool_dims', FIM_UNSUPPORTED,
            counted=False)
    return tuple(o.value for o in out)


def conv3d_weight(weight, mode):
    """The Conv3d weight [Cout, Cin, K, K, K] as the forward operand [Cin, K^3, Cout4] (mode 0) or the input-gradient operand
    [Cout, K^3, Cin4] (mode 1); entries of the derived-weight cache, their pad columns zero."""
    Cout, Cin, K = weight.shape[:3]
    return _permuted_weight('c3_q' if mode else 'c3_p', weight, (Cout, Cin, K))


def conv3d_pool_fwd(x, strides, wp, bias, imgs, Cin, D, H, W, Cout, K, P, St, cf_out, y, arg):
    """y / arg = elu(max over each pool cell of conv3d(x) + bias) and the cell's one-byte argmax (include/nnr_hip.h); strides = (image,
    channel, depth, row, column) of x in floats.  2 Cin K^3 flops per computed position and filter."""
    PD, PH, PW = conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St)
    if not _prof.active():
        L.check(L.lib().nnr_conv3d_pool_fwd(_p(x), *strides, _p(wp), _p(bias), imgs, Cin, D, H, W, Cout, K, P, St, int(cf_out), _p(y), _p(arg), _s()),
                   'nnr_conv3d_pool_fwd', FIM_UNSUPPORTED)
        return

    def flops(vals=None):
        return 2.0 * imgs * PD * PH * PW * P ** 3 * Cout * Cin * K ** 3
    flops.dyn = []
    flops.tag = 'imgs%d %dx%dx%dx%d->%d k%d p%d/%d' % (imgs, Cin, D, H, W, Cout, K, P, St)
    with _prof.span('conv3d_pool_fwd', flops):
        L.check(L.lib().nnr_conv3d_pool_fwd(_p(x), *strides, _p(wp), _p(bias), imgs, Cin, D, H, W, Cout, K, P, St, int(cf_out), _p(y), _p(arg), _s()),
                   'nnr_conv3d_pool_fwd', FIM_UNSUPPORTED)


def conv3d_pool_bwd(dy, y, arg, x, strides, wq, imgs, Cin, D, H, W, Cout, K, P, St, cf_out, dx, dw, db):
    """dw [Cout, Cin, K, K, K] and db [Cout] accumulate, dx (same strides as x, or None) is written; reproducible (include/nnr_hip.h)."""
    nws = L.lib().nnr_conv3d_pool_bwd_ws_floats(imgs, Cin, D, H, W, Cout, K, P, St)
    if nws == 0 and imgs > 0:
        raise L.NnrHipError('nnr_conv3d_pool_bwd: %s' % FIM_UNSUPPORTED)
    ws = torch.empty(max(1, nws), device=dy.device, dtype=torch.float32)
    tape_keep(ws)

    def launch():
        L.check(L.lib().nnr_conv3d_pool_bwd(_p(dy), _p(y), _p(arg), _p(x), *strides, _p(wq), imgs, Cin, D, H, W, Cout, K, P, St, int(cf_out), _p(dx),
                                               _p(dw), _p(db), _p(ws), _s()), 'nnr_conv3d_pool_bwd', FIM_UNSUPPORTED)
    if not _prof.active():
        return launch()
    PD, PH, PW = conv3d_pool_dims(Cin, D, H, W, Cout, K, P, St)

    def flops(vals=None):           # one position per (cell, filter): the weight gradient's taps, and as many again for the input gradient
        return 2.0 * imgs * PD * PH * PW * Cout * Cin * K ** 3 * (2 if dx is not None else 1)
    flops.dyn = []
    flops.tag = 'imgs%d %dx%dx%dx%d->%d k%d p%d/%d%s' % (imgs, Cin, D, H, W, Cout, K, P, St, '' if dx is not None else ' dw only')
    with _prof.span('conv3d_pool_bwd', flops):
        launch()


def fill_zero(t):
    """t.zero_() as an entry point of the library (hipMemsetAsync on the current stream): part of the launch tape."""
    assert t.is_contiguous()
    L.check(L.lib().nnr_fill_zero(_p(t), t.numel() * t.element_size(), _s()), 'nnr_fill_zero')
    return t


def copy_bytes(dst, src):
    """dst <- src (device to device, same byte size, both contiguous)."""
    nb = src.numel() * src.element_size()
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() * dst.element_size() == nb
    L.check(L.lib().nnr_copy_bytes(_p(dst), _p(src), nb, _s()), 'nnr_copy_bytes')
    return dst


def fill_column_u8(mask, col, value):
    """mask[:, col] = value for a contiguous 2-D bool / uint8 tensor (userEncoders.py:73)."""
    assert mask.dim() == 2 and mask.is_contiguous() and mask.element_size() == 1
    rows, cols = mask.shape
    L.check(L.lib().nnr_fill_column_u8(_p(mask), rows, cols, col % cols, value, _s()), 'nnr_fill_column_u8')


def transpose2d(x, out, rows, cols, accumulate=False):
    L.check(L.lib().nnr_transpose2d(_p(x), _p(out), rows, cols, accumulate, _s()), 'nnr_transpose2d')
