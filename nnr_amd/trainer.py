"""Inner training step of the reference's `Trainer.train` / `distributed_train` (trainer.py:81-120, 261-300):
forward, loss, zero_grad, backward, [gradient all-reduce], clip_grad_norm_(gradient_clip_norm), Adam.step -- with the
optimizer state in flat fp32 buffers and clip+Adam fused into one HBM-bound kernel.  The epoch loop, dev evaluation and
checkpoint bookkeeping of the reference are nnr_amd/run.py."""
import os

import torch
import torch.nn as nn

from . import dp, ops
from . import profile as _prof
from .model import negative_log_softmax

# NNR_NATIVE_STEP=0: always the autograd path (loss.backward() through the encoders' autograd Functions).
# NNR_REPLAY=0: the native step is issued call by call from Python every step (no tape).
_NATIVE_STEP = os.environ.get('NNR_NATIVE_STEP', '1') != '0'
_REPLAY = os.environ.get('NNR_REPLAY', '1') != '0'
# Data parallelism: NNR_REPLAY_DP=0 issues the native step call by call.  (Round 3: with the host callbacks of a replay -- torch.distributed's
# all-reduce between the tape's segments -- re-entered under torch.cuda.ExternalStream(raw handle), 4 of 12 two-rank runs of a
# tiny-dimension epoch ended with parameters that differed between the ranks or from the CPU checker: an ExternalStream is another stream
# IDENTITY for the same hardware queue, and c10d / the caching allocator order their copies and buffer reuse per identity.  Re-entered
# under the very Stream object that was current at recording time: 16 of 16 + the full two-rank test; profiles/r03a_dp_flaky.txt.)
_REPLAY_DP = os.environ.get('NNR_REPLAY_DP', '1') != '0'
def _tape_budget_gb(dev):
    e = os.environ.get('NNR_TAPE_MAX_GB')
    if e is not None:
        return float(e)
    try:
        return torch.cuda.get_device_properties(dev).total_memory / 2 ** 30 / 4.0
    except Exception:
        return 64.0


_SKIP_POLL = int(os.environ.get('NNR_SKIP_POLL', '8'))
_WARM_STEPS = 2          # eager steps before a tape is recorded (first-use allocations: workspaces, W^T copies, packed weights)


class FlatParams:
    """Re-homes every parameter of `model` (and its gradient) as a view into one flat fp32 buffer.
    Offsets are padded to 4 floats so every view is 16-byte aligned.  Device-agnostic (used by the gloo CPU tests too)."""

    def __init__(self, model: nn.Module):
        params = [p for p in model.parameters() if p.requires_grad]          # nn.Module dedups the shared news encoder
        # groups a module wants back to back (MultiHeadAttention: W_Q | W_K | W_V as one matrix) go first, in group order;
        # group members are multiples of 4 floats or the padding below would separate them (then the fused view is simply
        # not formed and the per-tensor path runs)
        grouped, seen = [], set()
        for m in model.modules():
            for g in getattr(m, 'adjacent_parameter_groups', lambda: [])():
                if all(q.requires_grad and id(q) not in seen for q in g):
                    grouped += g
                    seen.update(id(q) for q in g)
        params = grouped + [p for p in params if id(p) not in seen]
        self.params = params
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        dev = params[0].device
        self.flat = torch.zeros(total, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(total, device=dev, dtype=torch.float32)
        for p, o in zip(params, offs):
            n = p.numel()
            self.flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
        self.numel = total
        self.offsets = offs

    def zero_grad(self):
        if self.grad.is_cuda:
            ops.fill_zero(self.grad)
        else:
            self.grad.zero_()


class _Own:
    """The parameters a user encoder owns itself: its direct parameters and its children except the shared news encoder."""

    def __init__(self, ue, children):
        self.ue, self.children = ue, children

    def parameters(self):
        for p in self.ue.parameters(recurse=False):
            yield p
        for m in self.children:
            yield from m.parameters()


class _Const:
    """A launch's algorithmic FLOPs with the device-side sizes of ITS step bound (see Trainer._snapshot_sizes)."""

    def __init__(self, fn, value):
        self.value = value
        for k in ('tag', 'tn_dims', 'op_bytes', 'hbm', 'scale'):
            if hasattr(fn, k):
                setattr(self, k, getattr(fn, k))

    def __call__(self):
        return self.value


class Trainer:
    def __init__(self, model, config, native=None, replay=None):
        """native: run the CNE+SUE step as a plain sequence of C-ABI calls (nnr_amd.step) instead of through autograd (default: on,
        NNR_NATIVE_STEP); replay: record that sequence once per batch shape and replay it natively (nnr_amd.tape; default: on,
        NNR_REPLAY).  Models the native step does not cover (MHSA / CNN / ATT encoders, tie_order 'torch') take the autograd path."""
        self.model = model
        self.native = _NATIVE_STEP if native is None else bool(native)
        self.replay = (_REPLAY and (dp.world_size() == 1 or _REPLAY_DP)) if replay is None else bool(replay)
        self.tapes = {}              # batch-shape key -> nnr_amd.tape.Tape
        self._skipped_seen = None    # the library's skipped-step count (process-wide) when this trainer first polled / started
        self._skip_event = None      # HIP event behind the step NNR_SKIP_POLL steps back (train_step)
        self.skip_warnings = []      # (step_count at which it was noticed, library count) per warning
        self.unrecordable = set()    # batch-shape keys whose recording was discarded (tape.violations): they stay call by call
        self.tape_violations = []    # diagnostics: the violations of the last discarded recording
        self.native_steps = {}       # batch-shape key -> eager native steps run so far
        self.timing = False          # set by the caller (bench.py): the next step carries HIP events around its GEMM / recurrence calls
        self._snaps = {}             # tape -> [snapshot of the device-side sizes per timing replay]
        self.last_path = None        # 'autograd' | 'native' | 'record' | 'replay'  (diagnostics / tests)
        self.config = config
        self.flat = FlatParams(model)
        self.m = torch.zeros_like(self.flat.flat)
        self.v = torch.zeros_like(self.flat.flat)
        self.sumsq = torch.zeros(1, device=self.flat.flat.device, dtype=torch.float32)
        self.step_count = 0
        self.gradient_clip_norm = float(config.gradient_clip_norm)
        self.lr, self.weight_decay = float(config.lr), float(config.weight_decay)
        dp.broadcast_parameters(self.flat.flat)
        # bucketed exchange: the user encoder's own gradients are final first (its backward runs before the news encoder's)
        ue = getattr(model, 'user_encoder', None)
        own = [m for name, m in ue.named_children() if name != 'news_encoder'] if ue is not None else []
        ne = getattr(model, 'news_encoder', None)
        table = ne.word_embedding.weight if (ne is not None and hasattr(ne, 'word_embedding')) else None
        self.exchange = dp.GradientExchange(self.flat, early_modules=[_Own(ue, own)] if ue is not None else [], table_param=table)
        if ue is not None:
            ue.__dict__['_grads_ready_hook'] = self.exchange.early_ready
        if ne is not None:
            ne.__dict__['_table_scatter_hook'] = self.exchange.table_scatter_done      # (CNE calls it after each embedding-row scatter GEMM)
            ne.__dict__['_tokens_hook'] = self.exchange.note_tokens                     # (... and with each planned token stream: touched-row exchange)

    def train_step(self, batch):
        """One optimizer step on `batch` (21 device tensors, Model.forward order).  Returns (logits, loss) as device
        tensors -- no host synchronisation (the reference's float(loss) sync at trainer.py:115 is the caller's choice).

        Skipped optimizer steps (a recurrence exchange time-out poisons its tile with NaN, nnr_clip_adam then leaves the parameters
        untouched) are reported within 2 x NNR_SKIP_POLL steps (default 8 -> 16; 0 = never): the clip+Adam kernel mirrors the
        library's skipped-step count into pinned host memory, which is read after EVERY step without a synchronisation
        (nnr_adam_skipped_peek); every NNR_SKIP_POLL-th step the host additionally waits for the event recorded NNR_SKIP_POLL
        steps earlier (normally long complete), which bounds how far the host runs ahead of the device and so how stale the mirror
        can be.  (Round 4 polled a synchronous device read every 512 steps: up to 511 silently skipped steps.)"""
        gpu = batch[15].is_cuda
        if self._skipped_seen is None and gpu:
            self._skipped_seen = self.skipped_steps()          # baseline (the counter is process-wide); one sync at the first step
        out = self._train_step(batch)
        if _SKIP_POLL and gpu:
            if self.step_count % _SKIP_POLL == 0:
                prev, self._skip_event = self._skip_event, torch.cuda.Event()
                self._skip_event.record()
                if prev is not None:
                    prev.synchronize()                         # the step NNR_SKIP_POLL steps back is complete: its count is in the mirror
            n = self.skipped_peek()
            if n is not None and n > self._skipped_seen:
                import warnings
                warnings.warn('nnr_amd: %d optimizer step(s) skipped so far because the gradient norm was not finite (recurrence exchange time-outs: %d); '
                              'noticed at step %d' % (n, ops.lstm_sync_timeouts(), self.step_count))
                self._skipped_seen = n
                self.skip_warnings.append((self.step_count, n))
        return out

    def _train_step(self, batch):
        model = self.model
        if self.native and batch[15].is_cuda and model.training:
            from . import step as native_step
            if native_step.supported(model):
                return self._native_train_step(batch, native_step)
        self.last_path = 'autograd'
        self.exchange.begin_step(int(batch[0].shape[0]))
        self.flat.zero_grad()
        from . import step as native_step
        with native_step.matrix_path(model, batch):      # (same kernels as the native step of this model would run)
            logits = model(*batch)
            loss = negative_log_softmax(logits)
            # the encoders' regularisers (trainer.py:109-114); None for every encoder but OMAP
            if model.news_encoder.auxiliary_loss is not None:
                loss = loss + model.news_encoder.auxiliary_loss.mean()
            if model.user_encoder.auxiliary_loss is not None:
                loss = loss + model.user_encoder.auxiliary_loss.mean()
            loss.backward()
        ops.join_extra_streams()
        scale = self.exchange.finish()
        self.optimizer_step(scale)
        return logits.detach(), loss.detach()

    # ------------------------------------------------------------------------------------------------ native step / tape
    def _zero_grad_aside(self):
        """Clear the flat gradient buffer on the leaf stream: nothing writes a gradient before the backward pass, so the 100 MB fill
        leaves the head of the step's dependent chain (forward_backward waits for it via wait_grad_zeroed)."""
        dev = self.flat.grad.device
        leaf = ops.leaf_stream(dev)
        leaf.wait_stream(torch.cuda.current_stream(dev))        # behind the previous step's optimizer (it reads the gradients)
        with torch.cuda.stream(leaf):
            self.flat.zero_grad()
            self._zeroed = torch.cuda.Event()
            self._zeroed.record()

    def wait_grad_zeroed(self):
        ev, self._zeroed = getattr(self, '_zeroed', None), None
        if ev is not None:
            # (the other streams of the backward pass fork from this one, the leaf stream is ordered behind its own fill)
            torch.cuda.current_stream(self.flat.grad.device).wait_event(ev)

    def _body(self, batch, native_step):
        self.exchange.begin_step(int(batch[0].shape[0]))
        self._zero_grad_aside()
        logits, loss = native_step.forward_backward(self, batch)
        scale = self.exchange.finish()
        self.optimizer_step(scale)
        return logits, loss

    def _next_seeds(self):
        """The dropout seeds the next encoder calls will draw (NewsEncoder._next_seed / UserEncoder._next_seed)."""
        ne, ue = self.model.news_encoder, self.model.user_encoder
        return {'news_seed': (ne._seed_base + 104729 * (ne._calls + 1)) & 0x7FFFFFFF,
                'user_seed': (ue._seed_base + 15485863 * (ue._calls + 1)) & 0x7FFFFFFF}

    def _native_train_step(self, batch, native_step):
        return self._native_train_step_on_current(batch, native_step)

    def _native_train_step_on_current(self, batch, native_step):
        key = tuple((tuple(t.shape), t.dtype) for t in batch)
        tape = self.tapes.get(key)
        # scalars baked into the recorded arguments + the HIP stream the step is issued on (the tape replays on the recorded streams:
        # a caller that switches its current stream gets a fresh tape, not launches that are unordered with its own work)
        hyper = (self.lr, self.weight_decay, self.gradient_clip_norm, dp.world_size(), float(self.model.news_encoder.dropout_rate),
                 float(getattr(self.model.user_encoder, 'dropout_rate', 0.0)), torch.cuda.current_stream(self.flat.grad.device).cuda_stream)
        if tape is not None and tape.hyper != hyper:
            # something that is baked into the recording changed (learning rate, clip, weight decay, dropout rate, world size, the
            # caller's current stream): drop the tape and record a fresh one on the next step
            tape.close()
            del self.tapes[key]
            tape = None
        eager_profile = _prof._on                       # eager HIP-event spans requested (bench's isolated leg, tools): no tape
        if tape is not None and self.replay and not eager_profile and not ops.ONE_STREAM[0] and tape.matches(batch):
            values = self._next_seeds()
            self.model.news_encoder._calls += native_step.news_calls_per_step(self.model)      # the replayed calls consume the same per-call seeds the eager ones would
            self.model.user_encoder._calls += 1
            self.step_count += 1
            values['adam_step'] = self.step_count
            timing = self.timing and tape._nsets < 64
            tape.replay(values, batch, timing=timing)
            if timing:
                self._snapshot_sizes(tape)
            ops.PARAM_EPOCH[0] += 1
            self.last_path = 'replay'
            # tape.out are the recorded step's OWN logits / loss buffers, overwritten by the next replay: hand out copies, as the
            # call-by-call and autograd paths hand out fresh tensors (a loop that keeps `loss` for later -- epoch-loss lists, logging
            # every k steps -- would otherwise read the last step's values; round-3 advisor).  Two device-to-device copies of 1.3 KB.
            return tuple(ops.copy_bytes(torch.empty_like(t), t) for t in tape.out)
        n = self.native_steps.get(key, 0)
        self.native_steps[key] = n + 1
        can_record = (self.replay and tape is None and n >= _WARM_STEPS and not eager_profile and not ops.ONE_STREAM[0] and len(self.tapes) < 4
                      and not torch.cuda.is_current_stream_capturing() and key not in self.unrecordable and native_step.recordable(batch))
        tape = None
        if can_record:
            from .tape import Tape, TapeError
            try:
                tape = Tape(batch, self._next_seeds(), known=(self.flat.flat, self.flat.grad, self.m, self.v, self.sumsq))
            except TapeError:
                tape = None                             # (this step's two dropout seeds are too close to tell apart: record the next one)
        if tape is None:
            self.last_path = 'native'
            logits, loss = self._body(batch, native_step)
            return logits, loss
        tape.hyper = hyper
        try:
            out = tape.record(lambda: self._body(batch, native_step))
        except Exception:
            tape.close()
            raise
        if tape.violations:
            # the step itself ran eagerly and is complete; only the recording is unusable (a device pointer that belongs to neither the
            # batch, nor a buffer the tape keeps alive, nor the flat parameter / gradient / moment buffers reached a call): stay call by call
            import warnings
            warnings.warn('nnr_amd: launch tape discarded, %d recorded pointer(s) of unknown provenance (first: %s argument %s); this batch '
                          'shape stays on the call-by-call native step' % (len(tape.violations), tape.violations[0][0], tape.violations[0][1]))
            self.tape_violations = list(tape.violations)
            tape.close()
            self.unrecordable.add(key)
            self.last_path = 'native'
            return out
        # footprint bound (round-3 verdict): a tape pins every buffer of its step (14.5 GB at batch 64, ~29 GB at 128) for as long as it
        # lives; the tapes of one trainer together stay under NNR_TAPE_MAX_GB (default: a quarter of the device's memory), a batch shape
        # whose recording would exceed it stays on the call-by-call native step
        held = sum(t.info()['buffers_held_gb'] for t in self.tapes.values()) + tape.info()['buffers_held_gb']
        if held > _tape_budget_gb(batch[0].device):
            import warnings
            warnings.warn('nnr_amd: launch tape discarded, the tapes of this trainer would pin %.1f GB (limit %.1f GB, NNR_TAPE_MAX_GB); this batch '
                          'shape stays on the call-by-call native step' % (held, _tape_budget_gb(batch[0].device)))
            tape.close()
            self.unrecordable.add(key)
            self.last_path = 'native'
            return out
        tape.out = out
        self.tapes[key] = tape
        self.last_path = 'record'
        return tuple(ops.copy_bytes(torch.empty_like(t), t) for t in tape.out)

    def _snapshot_sizes(self, tape):
        """After a timing replay: copy the device-side sizes (live token counts) the timed launches depended on; the buffers are
        overwritten by the next step.  (A few 4-byte device copies on the step's stream, only on instrumented steps.)"""
        dyn = {}
        for _, fn in tape.tags:
            for t in getattr(fn, 'dyn', ()):
                dyn[t.data_ptr()] = t
        ptrs = list(dyn)
        snap = torch.stack([dyn[p].reshape(-1)[0] for p in ptrs]) if ptrs else None
        self._snaps.setdefault(tape, []).append((ptrs, snap))

    def collect_timings(self):
        """Move the HIP-event timings of every timing replay so far into nnr_amd.profile (synchronises)."""
        for tape, snaps in self._snaps.items():
            for (ptrs, snap), rec in zip(snaps, tape.timings()[-len(snaps):]):
                vals = dict(zip(ptrs, snap.tolist())) if snap is not None else {}
                for family, fn, ms in rec:
                    c = _Const(fn, float(fn(vals)))
                    if hasattr(fn, 'bytes_fn'):
                        c.op_bytes = fn.bytes_fn(vals)
                    _prof.TAPE_RECORDS.append((family, c, ms))
        self._snaps = {}

    def optimizer_step(self, grad_scale=1.0):
        self.step_count += 1
        # sum g^2 over the whole flat gradient in one pass (round 5: the table span's share taken early on a helper stream measured SLOWER,
        # profiles/r05_ab.txt)
        ops.sumsq(self.flat.grad, self.sumsq)
        ops.clip_adam(self.flat.flat, self.flat.grad, self.m, self.v, self.sumsq, grad_scale, self.gradient_clip_norm, self.lr, 0.9, 0.999,
                      1e-8, self.weight_decay, self.step_count)
        ops.PARAM_EPOCH[0] += 1       # parameters changed behind torch's back: invalidate the derived weights

    def skipped_steps(self, reset=False):
        """Optimizer steps dropped so far because the gradient norm was not finite (nnr_clip_adam leaves parameters and moments
        untouched for such a step; the reference's clip_grad_norm_ + Adam would go NaN, trainer.py:118-120).  A training loop polls
        this every few hundred steps and stops when it moves.  Synchronises.  (step_count, i.e. Adam's bias correction, still
        advances for a skipped step: the host cannot know without a sync; one step's drift of 1 - beta^t is below 1e-3 after step 7.)"""
        import ctypes as C
        from . import _lib as L
        v = C.c_uint()
        L.check(L.lib().nnr_adam_skipped_steps(C.byref(v), reset), 'nnr_adam_skipped_steps')
        return int(v.value)

    def skipped_peek(self):
        """The skipped-step count as of the last COMPLETED optimizer step -- no synchronisation (pinned host mirror written by the
        clip+Adam kernel); None when the mirror could not be set up (then only skipped_steps() works)."""
        import ctypes as C
        from . import _lib as L
        v = C.c_uint()
        if L.lib().nnr_adam_skipped_peek(C.byref(v)) != 0:
            return None
        return int(v.value)

    def grad_total_norm(self, grad_scale=1.0):
        s = torch.empty(1, device=self.flat.grad.device, dtype=torch.float32)
        ops.sumsq(self.flat.grad, s)
        return float(s.sqrt()) * grad_scale
