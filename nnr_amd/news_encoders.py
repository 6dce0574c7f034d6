"""News encoders of the hot path -- same class names, constructor signatures, parameter names and forward
signatures as the reference's newsEncoders.py, computed by the HIP kernels of libnnr_hip.so.

CNE (newsEncoders.py:57-141) pipeline per token stream (title L=32 / content L=128), all on packed valid tokens only:
  seq_plan  -> [embedding-row gather + dropout + x.W_ih^T + b]  (one GEMM, gather fused in the A loader)
            -> persistent Bi-LSTM recurrence (both streams, both directions, ONE launch)
            -> cross-selective gate  H * sigmoid(H.W_H^T + M(c_other))   (GEMM epilogue)
            -> additive self attention (GEMM with fused tanh.w2 row-dot) -> wave-softmax pool
            -> cross attention  score = <H~_t, K^T(Q q + b)> / sqrt(A)   (GEMV form) -> pool
            -> feature fusion with category / subCategory rows.
The backward pass is written by hand against the same kernels (no autograd graph inside the encoder); parameter
gradients are accumulated straight into `param.grad`.

The pipeline is driven by what a class keeps: `cne_streams` (title, content or both), `cne_gate` (the cross-selective gate with its rank
pairing) and `cne_cross` (the cross pools).  CNE keeps everything; the paper's ablations CNE_Title / CNE_Content / CNE_wo_CS / CNE_wo_CA
(variantEncoders.py) leave something out and issue the corresponding subset of CNE's launches.

Tie order (see oracle/nnr_oracle.py:length_order): the reference sorts each stream by length with an unstable sort and
gates the title at title-rank r with the content memory at content-rank r.  Because this implementation keeps each stream
in its own sorted order end to end, that pairing is reproduced by construction; `tie_order` only selects how equal lengths
are ordered: 'stable' (device-side, no host sync; = torch 1.12.1 CPU behaviour) or 'torch' (ask the installed torch on the
host, exactly as the reference's CPU path would -- costs a device->host sync, used for bit-parity tests)."""
import math
import os
import pickle

import torch
import torch.nn as nn

from . import ops
from .layers import Attention, CandidateAttention, ScaledDotProduct_CandidateAttention, MultiHeadAttention, Conv1D, Conv2D_Pool, LSTMParams, grad_of, personalized_attention

_SITE = dict(title=1, content=2, cat=3, sub=4)
_DP_TABLE_FIRST = int(os.environ.get('NNR_DP_TABLE_FIRST', '0'))       # 1: always, -1: when world_size > 1, 0 (default): never -- no multi-GPU box to measure it on


def _dp_world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_initialized() else 1


class NewsEncoder(nn.Module):
    """newsEncoders.py:11-54."""
    batch_independent = False            # True: a news representation does not depend on the other news of its call (evaluate.news_reps_cacheable)
    cne_gate = False                     # True: the call's sequences gate each other by sorted rank (CNE, CNE_wo_CA; evaluate.compute_scores_dedup)
    pad_dedup = True                     # False: Model.forward's inference de-duplication of PAD history slots does not apply
    tie_order = 'stable'                 # the order of equal lengths where sequences are sorted (the CNE family sets it from the config)

    def __init__(self, config, word_table=None):
        super().__init__()
        self.word_embedding_dim = config.word_embedding_dim
        self.word_embedding = nn.Embedding(num_embeddings=config.vocabulary_size, embedding_dim=self.word_embedding_dim)
        fname = 'word_embedding-' + str(config.word_threshold) + '-' + str(config.word_embedding_dim) + '-' + config.tokenizer + '-' + \
                str(config.max_title_length) + '-' + str(config.max_abstract_length) + '-' + config.dataset + '.pkl'
        if word_table is None and os.path.exists(fname):            # the reference's behaviour (newsEncoders.py:16-17)
            with open(fname, 'rb') as f:
                word_table = pickle.load(f)
        if word_table is not None:
            self.word_embedding.weight.data.copy_(word_table)
        self.category_embedding = nn.Embedding(num_embeddings=config.category_num, embedding_dim=config.category_embedding_dim)
        self.subCategory_embedding = nn.Embedding(num_embeddings=config.subCategory_num, embedding_dim=config.subCategory_embedding_dim)
        self.dropout_rate = float(config.dropout_rate)
        self.auxiliary_loss = None
        self._seed_base = int(getattr(config, 'seed', 0)) * 7919 + 17
        self._calls = 0

    def _next_seed(self):
        self._calls += 1
        return (self._seed_base + 104729 * self._calls) & 0x7FFFFFFF

    def initialize(self):
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)
        nn.init.uniform_(self.subCategory_embedding.weight, -0.1, 0.1)
        with torch.no_grad():
            self.subCategory_embedding.weight[0].zero_()

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        raise Exception('Function forward must be implemented at sub-class')

    def conv_text(self, text, conv, n, Lx, p, seed, image=False):
        """The CNN family's text front [n*L, C]: dropout(word rows, seed + 1) -> Conv1d + ReLU -> dropout_(seed + 2); the convolution as k
        shifted GEMMs or, with `image`, as one padded-row product (functional.Conv1dImageFn)."""
        from . import functional as Fn
        table = self.word_embedding.weight
        if image:
            c = Fn.Conv1dImageFn.apply(table, text, conv, n, Lx, p, seed + 1, torch.is_grad_enabled() and table.requires_grad)
        else:
            c = Fn.Conv1dReluFn.apply(Fn.EmbedDropFn.apply(table, text, p, seed + 1), conv, n, Lx)
        return Fn.DropoutFn.apply(c, p, seed + 2)


# ================================================================================================== CNE
class _CNEPairFunction(torch.autograd.Function):
    """Candidate call + history call of the SAME encoder in one pass.  Default: both calls planned as ONE packed token stream
    (cne union: every per-token kernel runs once over both calls; the rank pairing of newsEncoders.py:128-129 stays per call
    through nnr_cne_pair_map).  _CNE_UNION = False (tests): two lock-step calls that only share the recurrence launches."""

    @staticmethod
    def forward(ctx, anchor, mod, *tensors):
        ctx.mod = mod
        if _CNE_UNION:
            ((rep_a, rep_b), sv), = cne_forward_many(mod, [tuple(zip(tensors[:6], tensors[6:]))])
            ctx.saved = (sv,)
            return rep_a, rep_b
        (rep_a, sv_a), (rep_b, sv_b) = cne_forward_many(mod, [tensors[:6], tensors[6:]])
        ctx.saved = (sv_a, sv_b)
        return rep_a, rep_b

    @staticmethod
    def backward(ctx, drep_a, drep_b):
        if len(ctx.saved) == 1:
            sv, = ctx.saved
            D = drep_a.shape[-1]
            drep = torch.cat([drep_a.reshape(-1, D), drep_b.reshape(-1, D)])
            cne_backward_many(ctx.mod, [(sv, drep)])
        else:
            sv_a, sv_b = ctx.saved
            cne_backward_many(ctx.mod, [(sv_a, drep_a.contiguous()), (sv_b, drep_b.contiguous())])
        ctx.saved = None
        return (None,) * 14


class _CNEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, mod, title_text, title_mask, content_text, content_mask, category, subCategory):
        rep, saved = cne_forward(mod, title_text, title_mask, content_text, content_mask, category, subCategory)
        ctx.mod, ctx.saved = mod, saved
        return rep

    @staticmethod
    def backward(ctx, drep):
        cne_backward(ctx.mod, ctx.saved, drep.contiguous())
        ctx.saved = None
        return (None,) * 8


def cne_forward(mod, title_text, title_mask, content_text, content_mask, category, subCategory):
    """Single encoder call (plugin API).  Model.forward uses cne_forward_many to share the recurrence launch between the
    candidate call and the history call."""
    (rep, saved), = cne_forward_many(mod, [(title_text, title_mask, content_text, content_mask, category, subCategory)])
    return rep, saved


_SIDE = {}
ops.STREAM_CACHES.append(_SIDE)
_LEAF2_ROWS = 65536         # the title stream's weight gradients on the second leaf stream up to this many content token rows (see _cne_bwd_pre)
_CNE_UNION = True           # candidate + history call as one packed token stream (tests switch it off: the two-call plugin path)


def _side_stream(dev):
    """One extra HIP stream per device for the small (candidate) encoder call."""
    key = (dev.type, dev.index)
    if key not in _SIDE:
        _SIDE[key] = ops.new_stream(dev)
    return _SIDE[key]


def _title_stream(dev):
    key = (dev.type, dev.index, 2)
    if key not in _SIDE:
        _SIDE[key] = ops.new_stream(dev)
    return _SIDE[key]


def _two_chains(dev, enable, title_fn, content_fn):
    """The title and the content chain of ONE encoder call are independent between their exchange points (c_n before the
    gate, the self-attention vectors before the cross attention and their gradients on the way back): on the big call the
    title chain runs on a third HIP stream next to the content chain.  Half of the step at batch 64 (7 of 16 ms) is the
    latency of dependent launches, not throughput; the title kernels are a quarter of the content kernels' size."""
    if not enable:
        title_fn()
        content_fn()
        return
    main = torch.cuda.current_stream(dev)
    s2 = _title_stream(dev)
    s2.wait_stream(main)
    with torch.cuda.stream(s2):
        title_fn()
    content_fn()
    main.wait_stream(s2)


class _on:
    """Run a phase of call #0 on the side stream when there are several calls; main-stream phases pass through."""

    def __init__(self, side):
        self.side = side

    def __enter__(self):
        if self.side is not None:
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.side is not None:
            self.ctx.__exit__(*a)


def _fork_join(n_calls, dev, phase):
    """phase(i) for every call: call 0 (the candidates: ~10 % of the rows, launch-latency-bound kernels) on the side stream,
    concurrently with the other calls on the current stream; returns after both streams are joined."""
    if n_calls == 1:
        return [phase(0, True)]
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        first = phase(0, False)
    rest = [phase(i, True) for i in range(1, n_calls)]
    main.wait_stream(side)
    return [first] + rest


def cne_forward_many(mod, calls):
    """Run several independent CNE calls in lock-step: everything is per call except the Bi-LSTM recurrence, which is ONE
    launch over all streams of all calls (it is latency-bound by its longest sequence, not throughput-bound).  The per-call
    phases of the first (small) call run on a second HIP stream, filling the gaps of the big call's kernels."""
    H, E = mod.hidden_dim, mod.word_embedding_dim
    dev = (calls[0][0][0] if isinstance(calls[0][0], tuple) else calls[0][0]).device
    lstms = tuple(getattr(mod, k + '_lstm') for k in mod.cne_streams)
    if len(calls) > 1:
        for lstm in lstms:                              # (re)pack on the main stream BEFORE forking: both calls read them
            ops.lstm_pack(lstm, H, E)
    else:
        # one call (the union of candidate and history call): the re-packs run on the leaf stream next to the planner / row gather
        ops.lstm_prefetch(dev, lstms, H, E)
    if mod.training:
        # the bf16 images of the parameters (and of their cached transposes) the gate / attention / user-encoder GEMMs will read: re-split on the LEAF
        # stream HERE -- behind the weight packing (which the input projection waits for: in front of it the splits cost +0.3 ms) and in FRONT of the
        # token sorts (needed by the backward pass only), i.e. under the input projection.  (Under the forward recurrence, whose workgroups fill every
        # CU, the 29 launches of ~5 us crawled at 70-160 us each and ended level with their first users: profiles/r06_ab.txt, first collection of the round.)
        ops.bx3_prefetch(dev)
    pre = _fork_join(len(calls), dev, lambda i, on_main: _cne_fwd_pre(mod, *calls[i], par=on_main))
    items = [sv['streams'][k] for k in reversed(range(len(mod.cne_streams))) for sv in pre]      # content streams first
    for i in range(0, len(items), 4):
        ops.lstm_fwd(items[i:i + 4], H)
    return _fork_join(len(calls), dev, lambda i, on_main: _cne_fwd_post(mod, pre[i], on_main))


def _torch_tie_perm(masks):
    """tie_order='torch': the installed torch's CPU sort decides the order of equal lengths, per call (as the reference's
    torch.sort calls do); for a union of calls, any length-descending order that keeps each call's own order."""
    perms, lens = [], []
    base = 0
    for m in masks:
        l = (m.sum(dim=1).long() + (~m[:, 0]).long()).cpu()      # lengths after the mask[:,0]=1 fix
        q = torch.sort(l, descending=True)[1]
        perms.append(q + base)
        lens.append(l[q])
        base += m.shape[0]
    if len(perms) == 1:
        return perms[0].to(torch.int32)
    q, l = torch.cat(perms), torch.cat(lens)
    return q[torch.sort(l, descending=True, stable=True)[1]].to(torch.int32)


def _cne_fwd_pre(mod, title_text, title_mask, content_text, content_mask, category, subCategory, par=False, partner=None):
    """partner (optional, single call only): (pc_of_title, pt_of_content) int64 [n] -- for sequence i, the sequence whose CONTENT
    memory gates title i / whose TITLE memory gates content i -- instead of the call's own rank pairing (see cne_history_dedup)."""
    union = isinstance(title_text, tuple)            # (candidate call's tensor, history call's tensor) per argument
    if union:
        B, N = title_text[0].shape[:2]
        n0 = B * N
        n = n0 + B * title_text[1].shape[1]
        dev = title_text[0].device
    else:
        B, N = title_text.shape[:2]
        n = n0 = B * N
        dev = title_text.device
    H, E, A = mod.hidden_dim, mod.word_embedding_dim, mod.attention_dim
    H2 = 2 * H
    f32 = dict(device=dev, dtype=torch.float32)
    p = mod.dropout_rate if mod.training else 0.0
    seed = mod._next_seed()
    emb = mod.word_embedding.weight

    kinds = mod.cne_streams
    streams = [None] * len(kinds)

    def prepare(slot, name, ids, mask, Lx):
        lstm, satt = getattr(mod, name + '_lstm'), getattr(mod, name + '_self_attention')
        Hlin, Mlin = (getattr(mod, name + '_H'), getattr(mod, name + '_M')) if mod.cne_gate else (None, None)
        catt = getattr(mod, name + '_cross_attention') if mod.cne_cross else None
        parts = list(zip(ids, mask)) if union else [(ids, mask)]
        ids2 = [ops.ids32(i, -1, Lx) for i, _ in parts]
        mask2 = [m.view(-1, Lx) for _, m in parts]      # views: the in-place mask[:,0]=1 must reach the caller's tensors
        perm = _torch_tie_perm(mask2).to(dev) if mod.tie_order == 'torch' else None
        plan = ops.SeqPlan(mask2[0], ids2[0], perm, *((mask2[1], ids2[1]) if union else ()))
        plan_ev = None
        if union and name == 'content' and mod.cne_gate:
            plan_ev = torch.cuda.Event()
            plan_ev.record()
        w = ops.lstm_pack(lstm, H, E)
        cap = plan.cap
        st = dict(name=name, L=Lx, plan=plan, plan_ev=plan_ev, w=w, lstm=lstm, Hlin=Hlin, Mlin=Mlin, satt=satt, catt=catt, seed=seed + _SITE[name])
        st['gates'] = torch.empty((cap, 2 * w.NP), **f32)
        # dropout(embedding rows) materialised ONCE per token (6 TB/s gather): fused into the GEMM's A loader the counter hash
        # is recomputed by each of the 21 column blocks (-16 % on this GEMM and on the dW_ih GEMM of the backward)
        st['xd'] = ops.embed_gather(emb, plan.tok, p, st['seed'], dyn=plan.total)
        hook = mod.__dict__.get('_tokens_hook')
        if hook is not None and (mod.training or torch.is_grad_enabled()):
            # data parallel: the touched-row exchange of the table gradient learns this stream's words -- whenever a backward pass may
            # follow (also an eval-mode gradient check: the backward's table hook is unconditional; round-5 advisor)
            hook(plan.tok, plan.total)
        if mod.training and E <= 320:
            # the backward's embedding-row gradient is a segmented reduction over the rows sorted by word id (reproducible, no atomic
            # ceiling): the sort needs only the planned ids and runs on the leaf stream under the forward pass
            st['tsort'] = ops.TokenSort(plan.tok, plan.total, emb.shape[0])
        ops.gemm(st['xd'], w.w_ihp, st['gates'], M=cap, N=2 * w.NP, K=E, lda=E, ldb=E, ldc=2 * w.NP, dyn=plan.total, dyn_dim=1, bias=w.b_p,
                 flop_scale=4.0 * H / w.NP)
        st['cell'] = torch.empty((cap, 2 * w.HP), **f32)
        st['hout'] = torch.empty((cap, H2), **f32)
        st['cn'] = torch.empty((n, H2), **f32)
        streams[slot] = st

    # the title and the content stream are independent up to the recurrence: plan + gather + input projection of the
    # (small) title stream run next to the content stream's on the big call
    # (a variant without one of the streams never looks at that stream's text and mask: not planned, not gathered, not written)
    inputs = dict(title=(title_text, title_mask, mod.max_title_length), content=(content_text, content_mask, mod.max_content_length))
    if len(kinds) == 2:
        _two_chains(dev, par, lambda: prepare(0, 'title', *inputs['title']), lambda: prepare(1, 'content', *inputs['content']))
    else:
        prepare(0, kinds[0], *inputs[kinds[0]])
    sv = dict(streams=streams, n=n, n0=n0, union=union, B=B, N=N, p=p, seed=seed, category=category, subCategory=subCategory)
    if union and mod.cne_gate:
        # rank pairing (newsEncoders.py:128-129): inside ONE call the partner of sorted position r is the other stream's position r;
        # in a union of two calls it is the other stream's position with the same (call, position inside the call).  Needs both
        # plans and nothing else: issued on the title stream behind the title projection, it is done long before the recurrence ends
        s2 = _title_stream(dev)
        with torch.cuda.stream(s2):
            s2.wait_event(streams[1]['plan_ev'])
            sv['pm'] = ops.cne_pair_map(streams[0]['plan'], streams[1]['plan'])
        sv['pm_stream'] = s2
    if partner is not None:
        assert not union and mod.cne_gate
        pc_t, pt_c = partner
        pt, pc = streams[0]['plan'], streams[1]['plan']
        # title at sorted position s is sequence order_t[s]; its partner content is sequence pc_t[.], at content position rank_c[.]
        sv['pm_override'] = (pc.rank.long()[pc_t[pt.order.long()]].to(torch.int32).contiguous(),
                             pt.rank.long()[pt_c[pc.order.long()]].to(torch.int32).contiguous())
    return sv


def _cne_fwd_post(mod, sv, par=False):
    sts = sv['streams']
    gate, cross, two = mod.cne_gate, mod.cne_cross, len(sts) == 2
    n, B, N, p, seed = sv['n'], sv['B'], sv['N'], sv['p'], sv['seed']
    dev = sts[0]['gates'].device
    H, E, A = mod.hidden_dim, mod.word_embedding_dim, mod.attention_dim
    H2 = 2 * H
    D = mod.news_embedding_dim
    f32 = dict(device=dev, dtype=torch.float32)

    if gate:
        if sv['union']:
            torch.cuda.current_stream(dev).wait_stream(sv['pm_stream'])
        sts[0]['pm'], sts[1]['pm'] = sv['pm'] if sv['union'] else sv.get('pm_override', (None, None))
    # cn_override (de-duplicated evaluation, evaluate.compute_scores_dedup): ((content memories [U, 2H], row per TITLE sorted position),
    # (title memories [U, 2H], row per CONTENT sorted position)) -- the gate reads its partner's memory from a table of the split's
    # distinct news instead of this call's own cn.  Forward only: set by that one caller on a call it made itself, never saved.
    cn_override = sv.get('cn_override') if gate else None
    # without the cross pools the self pools' vectors ARE the representation's leading columns: pooled straight into them
    rep = None if cross else torch.empty((n, D), **f32)

    def self_pool(st, col0):
        plan, cap, sa = st['plan'], st['plan'].cap, st['satt']
        st['th'] = torch.empty((cap, A), **f32)
        ops.gemm(st['Ht'], sa.affine1.weight, st['th'], M=cap, N=A, K=H2, lda=H2, ldb=H2, ldc=A, dyn=plan.total, dyn_dim=1,
                 bias=sa.affine1.bias, act=ops.ACT_TANH)
        st['alpha_s'] = torch.empty(cap, **f32)
        st['selfv'] = torch.empty((n, H2), **f32) if cross else rep[:, col0:col0 + H2]
        ldo = H2 if cross else D
        if A <= 256 and A % 4 == 0:
            # the w2 . tanh(.) score is computed inside the pool's own pass over the tokens (one launch less on the chain)
            ops.pool_fwd(x=st['Ht'], ldx=H2, D=H2, n=n, Lx=st['L'], plan=plan, th=st['th'], w2=sa.affine2.weight, alpha=st['alpha_s'],
                         out=st['selfv'], ldo=ldo)
        else:
            score = torch.empty(cap, **f32)
            ops.rowdot(st['th'], sa.affine2.weight, score, dyn=plan.total)
            ops.pool_fwd(x=st['Ht'], ldx=H2, D=H2, n=n, Lx=st['L'], plan=plan, score=score, alpha=st['alpha_s'], out=st['selfv'], ldo=ldo)

    def gate_and_self(st, other, col0):
        plan, cap = st['plan'], st['plan'].cap
        if not gate:
            st['Ht'] = st['hout']                        # the attention pools read the raw Bi-LSTM rows
            return self_pool(st, col0)
        # title_M(sorted_content_m): both indexed by sorted RANK (newsEncoders.py:128-129)
        if cn_override is not None:
            table, rows = cn_override[0 if st is sts[0] else 1]
            st['mproj'] = torch.empty((n, H2), **f32)
            ops.gemm(table, st['Mlin'].weight, st['mproj'], M=n, N=H2, K=H2, lda=table.stride(0), ldb=H2, ldc=H2, bias=st['Mlin'].bias, a_idx=rows)
        else:
            st['mproj'] = ops.linear_fwd(other['cn'], st['Mlin'].weight, st['Mlin'].bias, **({} if st['pm'] is None else {'a_idx': st['pm']}))
        st['G'] = torch.empty((cap, H2), **f32)
        st['Ht'] = torch.empty((cap, H2), **f32)
        ops.gemm(st['hout'], st['Hlin'].weight, st['Ht'], M=cap, N=H2, K=H2, lda=H2, ldb=H2, ldc=H2, dyn=plan.total, dyn_dim=1,
                 rowvec=st['mproj'], ldrv=H2, rowvec_map=plan.row_seq, act=ops.ACT_SIGMOID, aux_out=st['G'], ldaux=H2,
                 mul=st['hout'], ldmul=H2)
        self_pool(st, col0)

    if two:
        t_, c_ = sts
        _two_chains(dev, par, lambda: gate_and_self(t_, c_, 0), lambda: gate_and_self(c_, t_, H2))
    else:
        gate_and_self(sts[0], None, 0)

    if cross:
        rep = torch.empty((n, D), **f32)

    def cross_pool(st, other, col0):
        plan, ca = st['plan'], st['catt']
        st['qv'] = ops.linear_fwd(other['selfv'], ca.Q.weight, ca.Q.bias)                    # [n, A]
        st['v'] = torch.empty((n, H2), **f32)
        ops.gemm(st['qv'], ca.K.weight, st['v'], M=n, N=H2, K=A, lda=A, ldb=H2, ldc=H2, trans_b=True)   # K^T (Q q + b)
        st['alpha_c'] = torch.empty(plan.cap, **f32)
        ops.pool_fwd(x=st['Ht'], ldx=H2, D=H2, n=n, Lx=st['L'], plan=plan, v=st['v'], ldv=H2, scale=1.0 / math.sqrt(A),
                     alpha=st['alpha_c'], out=rep[:, col0:], ldo=D, add_in=st['selfv'], ldadd=H2)

    if cross:
        _two_chains(dev, par, lambda: cross_pool(t_, c_, 0), lambda: cross_pool(c_, t_, H2))
    # feature fusion (newsEncoders.py:50-54): category + subCategory rows of both calls in ONE launch, the two calls' id tensors read
    # where they lie (round 2: torch.cat x 2 + two launches)
    if sv['union']:
        cat0, cat1 = (ops.ids32(x, -1) for x in sv.pop('category'))
        sub0, sub1 = (ops.ids32(x, -1) for x in sv.pop('subCategory'))
    else:
        cat0, cat1 = ops.ids32(sv.pop('category'), n), None
        sub0, sub1 = ops.ids32(sv.pop('subCategory'), n), None
    cd, sd = mod.category_embedding.weight.shape[1], mod.subCategory_embedding.weight.shape[1]
    ops.fusion_rows_fwd(mod.category_embedding.weight, mod.subCategory_embedding.weight, cat0, sub0, cat1, sub1, rep[:, len(sts) * H2:], D, p,
                        seed + _SITE['cat'], seed + _SITE['sub'])
    sv.update(cats=(cat0, sub0, cat1, sub1), cd=cd, sd=sd)
    for st in sts if gate else ():                       # not needed by backward
        st.pop('mproj')
    if sv['union']:
        n0 = sv['n0']
        return (rep[:n0].view(B, N, D), rep[n0:].view(B, (n - n0) // B, D)), sv
    return rep.view(B, N, D), sv


def cne_backward(mod, sv, drep):
    cne_backward_many(mod, [(sv, drep)])


def cne_backward_many(mod, pairs):
    """Backward of cne_forward_many: per-call stages (call 0 on the side stream) around ONE shared recurrence-backward launch."""
    H = mod.hidden_dim
    dev = pairs[0][1].device
    for q in mod.parameters():          # materialise (zero-fill) missing .grad buffers on the main stream BEFORE forking
        grad_of(q)
    mod.__dict__['_table_scatters'] = len(mod.cne_streams) * len(pairs)      # embedding-row scatter GEMMs of this pass (one per stream and call)
    with ops.leaf_scope(dev) as leaf:        # weight-gradient GEMMs of the pre phase: leaves, joined after the recurrence + post phase
        _cne_bwd_rest(mod, pairs, H, dev, leaf)


def _cne_bwd_rest(mod, pairs, H, dev, leaf):
    _fork_join(len(pairs), dev, lambda i, on_main: _cne_bwd_pre(mod, pairs[i][0], pairs[i][1], on_main, leaf))

    # recurrence backward: one launch per stream kind on two HIP streams -- the title streams' on the side stream next to the content
    # streams' --, each followed by that kind's token-reduction GEMMs (batch 8: 4.68 vs 4.93 ms with ONE launch over every token stream;
    # batch 64: no difference).  All parameter-gradient accumulation below is atomic.
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)

    def run_kind(kind, kind_leaf):
        ops.lstm_bwd([sv['streams'][kind] for sv, _ in pairs], H)
        for sv, _ in pairs:
            _cne_bwd_post(mod, sv, sv['streams'][kind], kind_leaf)

    if len(mod.cne_streams) == 1:            # one stream kind: its launch on this stream, its weight gradients split with the leaf stream
        return run_kind(0, leaf)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        run_kind(0, None)
    run_kind(1, leaf)
    main.wait_stream(side)


def _cne_bwd_pre(mod, sv, drep, par=False, leaf=None):
    if leaf is None:
        leaf = lambda fn, *tensors, **kw: fn()
    sts = sv['streams']
    gate, cross, two = mod.cne_gate, mod.cne_cross, len(sts) == 2
    t_, c_ = sts if two else (sts[0], None)
    n, p, seed = sv['n'], sv['p'], sv['seed']
    H, E, A = mod.hidden_dim, mod.word_embedding_dim, mod.attention_dim
    H2 = 2 * H
    D = mod.news_embedding_dim
    dev = drep.device
    f32 = dict(device=dev, dtype=torch.float32)
    drep = drep.reshape(n, D)
    emb = mod.word_embedding.weight

    # (a leaf of the backward pass: nothing downstream reads the two table gradients -- on the leaf stream, off the dependent chain)
    leaf(lambda: ops.fusion_rows_bwd(*sv['cats'], sv['cd'], sv['sd'], drep[:, len(sts) * H2:], D, grad_of(mod.category_embedding.weight),
                                     grad_of(mod.subCategory_embedding.weight), p, seed + _SITE['cat'], seed + _SITE['sub']), drep)

    # the title stream's weight-gradient GEMMs on a SECOND leaf stream when the step is small and latency-bound (content stream <= 64 k token
    # rows = per-GPU batch 8: the leaf stream was the last to finish, 3.27-3.31 -> 3.23-3.24 ms); at batch 16 neutral, at batch 64 -- where the
    # leaf work is throughput-bound -- 0.1 ms SLOWER (10.72-10.77 vs 10.61-10.65), hence the bound
    def alt_leaf(st):
        return two and st['name'] == 'title' and c_['plan'].cap <= _LEAF2_ROWS

    # ---- cross attention pools: dv -> K / Q params and the gradient of the OTHER stream's self vector.  This pass does not write dHt:
    # it leaves its per-token d score (ds_c) behind, and the self pool's backward below writes dHt = alpha_s d self + alpha_c d cross +
    # scale ds_c v in ONE store (3 passes over [tokens, 400] for the two pools instead of 5; the cross pool must still run first, its dv
    # feeds the other stream's self vector)
    def cross_bwd(st, other, col0):
        plan, ca, cap = st['plan'], st['catt'], st['plan'].cap
        dv = torch.empty((n, H2), **f32)
        st['ds_c'] = torch.empty(cap, **f32)
        ops.pool_bwd(x=st['Ht'], ldx=H2, D=H2, n=n, Lx=st['L'], plan=plan, v=st['v'], ldv=H2, scale=1.0 / math.sqrt(A),
                     alpha=st['alpha_c'], dout=drep[:, col0:], lddo=D, dscore=st['ds_c'], dv=dv, lddv=H2)
        dqv = torch.empty((n, A), **f32)
        ops.gemm(dv, ca.K.weight, dqv, M=n, N=A, K=H2, lda=H2, ldb=H2, ldc=A)                 # dqv = dv . K^T
        leaf(lambda: (ops.linear_bwd_weight(st['qv'], dv, grad_of(ca.K.weight)),             # dK[A,H2] += qv^T dv
                      ops.linear_bwd_weight(dqv, other['selfv'], grad_of(ca.Q.weight), db=grad_of(ca.Q.bias))), dv, dqv, alt=alt_leaf(st))      # (bias gradient fused: column sums of dqv)
        other['dself_x'] = ops.linear_bwd_data(dqv, ca.Q.weight)                              # grad of other.selfv via the query

    if cross:
        _two_chains(dev, par, lambda: cross_bwd(t_, c_, 0), lambda: cross_bwd(c_, t_, H2))

    # ---- self attention pools, additive score, gate
    def self_gate_bwd(st, other, col0):
        plan, sa, cap = st['plan'], st['satt'], st['plan'].cap
        ds = torch.empty(cap, **f32)
        st['dHt'] = torch.empty((cap, H2), **f32)
        if cross:
            ops.pool_bwd(x=st['Ht'], ldx=H2, D=H2, n=n, Lx=st['L'], plan=plan, score=None, alpha=st['alpha_s'],
                         dout=drep[:, col0:], lddo=D, dout2=st['dself_x'], lddo2=H2, dx=st['dHt'], lddx=H2, dscore=ds,
                         alpha_b=st['alpha_c'], dout_b=drep[:, col0:], lddo_b=D, dscore_b=st['ds_c'], v_b=st['v'], ldv_b=H2, scale_b=1.0 / math.sqrt(A))
            st['ds_c'] = None
        else:
            ops.pool_bwd(x=st['Ht'], ldx=H2, D=H2, n=n, Lx=st['L'], plan=plan, score=None, alpha=st['alpha_s'],
                         dout=drep[:, col0:], lddo=D, dx=st['dHt'], lddx=H2, dscore=ds)
        th = st['th']
        ops.tanh_score_bwd(th, ds, sa.affine2.weight, grad_of(sa.affine2.weight), plan, A)    # th := dpre
        if not gate:
            # Ht is the recurrence's own output: dH = dHt + d tanh-projection . W1, the pool's store followed by an accumulating product
            st['dH'], st['dHt'] = st['dHt'], None
            ops.gemm(th, ops.wt(sa.affine1.weight), st['dH'], M=cap, N=H2, K=A, lda=A, ldb=A, ldc=H2, accumulate=True, dyn=plan.total, dyn_dim=1)
            leaf(lambda: ops.linear_bwd_weight(th, st['hout'], grad_of(sa.affine1.weight), dyn=plan.total, db=grad_of(sa.affine1.bias)), th, st['hout'],
                 alt=alt_leaf(st))
            return
        st['dH'] = torch.empty((cap, H2), **f32)
        dpre = torch.empty((cap, H2), **f32)             # (not Ht's buffer: the deferred weight-gradient GEMM below still reads it)
        # the GEMM that completes dHt (+= d tanh-projection . W1) applies the gate's backward in its epilogue: Ht = hout * G ->
        # dH = dHt * G, d pre = dHt * hout * G * (1 - G) -- one launch and one pass over dHt less on the dependent chain (round 4)
        ops.gemm(th, ops.wt(sa.affine1.weight), st['dH'], M=cap, N=H2, K=A, lda=A, ldb=A, ldc=H2, dyn=plan.total, dyn_dim=1,
                 pre_add=st['dHt'], ldpre=H2, gate_bwd=True, mul=st['G'], ldmul=H2, resid=st['hout'], ldres=H2, aux_out=dpre, ldaux=H2)
        leaf(lambda: ops.linear_bwd_weight(th, st['Ht'], grad_of(sa.affine1.weight), dyn=plan.total, db=grad_of(sa.affine1.bias)), th, st['Ht'], alt=alt_leaf(st))
        ops.gemm(dpre, ops.wt(st['Hlin'].weight), st['dH'], M=cap, N=H2, K=H2, lda=H2, ldb=H2, ldc=H2, accumulate=True,   # NT on W_H^T
                 dyn=plan.total, dyn_dim=1)
        leaf(lambda: ops.linear_bwd_weight(dpre, st['hout'], grad_of(st['Hlin'].weight), dyn=plan.total), dpre, st['hout'], alt=alt_leaf(st))
        dP = torch.empty((n, H2), **f32)                  # d mproj[rank]
        ops.packed_seq_sum(dpre, H2, plan, dP)
        pm, opm = st['pm'], other['pm']                   # union of two calls: mproj[s] = M(cn_other[pm[s]])  (pm^-1 = other's pm)
        leaf(lambda: ops.linear_bwd_weight(dP, other['cn'], grad_of(st['Mlin'].weight), db=grad_of(st['Mlin'].bias),
                                           **({} if pm is None else {'b_idx': pm})), dP, alt=alt_leaf(st))
        # (this [n, 400] x [400, 400] product runs beside the leaf stream's weight-gradient GEMMs and its automatic 74 KB tile waits for them:
        #  277 us in the step against 40 us alone.  The 19 KB register-staged tile halves its in-step time but leaves the step where it was --
        #  the chain waits for the same leaf work one call later; profiles/r06_ab.txt call 24 --, so the automatic choice stays)
        other['dcn'] = ops.linear_bwd_data(dP, st['Mlin'].weight, **({} if opm is None else {'a_idx': opm}))   # [n, H2], rank-indexed
        st['dHt'] = None

    if two:
        _two_chains(dev, par, lambda: self_gate_bwd(t_, c_, 0), lambda: self_gate_bwd(c_, t_, H2))
    else:
        self_gate_bwd(t_, None, 0)

    for st in sts:
        st['dh'] = st['dH']


def _cne_bwd_post(mod, sv, st, leaf=None):
    """After the recurrence backward of token stream `st`: weight / bias gradients of the LSTM and the embedding-row scatter.
    All of it is leaf work; with `leaf` given the three weight-gradient GEMMs go to the leaf stream and run next to the scatter
    GEMM (each has a partially filled last wave of workgroups that the other fills)."""
    p = sv['p']
    H, E = mod.hidden_dim, mod.word_embedding_dim
    H2 = 2 * H
    f32 = dict(device=st['gates'].device, dtype=torch.float32)
    emb = mod.word_embedding.weight
    plan, w, cap = st['plan'], st['w'], st['plan'].cap
    dg = st['gates']                                  # now d(pre-activation gates), p-order
    NP = w.NP

    # packed LSTM weight-gradient accumulators: one persistent, zeroed workspace per (token stream, encoder call); the unpack
    # kernel hands it back zeroed (three fill launches per stream and step otherwise -- 0.5 ms of kernel time in round 1)
    ws = mod.__dict__.setdefault('_dw_ws', {})
    key = (st['name'], sv['n'])
    if key not in ws or ws[key][0].shape != (2 * NP, E) or ws[key][0].device != dg.device:
        ws[key] = (torch.zeros((2 * NP, E), **f32), torch.zeros(2 * NP, **f32), torch.zeros((2, NP, H), **f32))
    dw_ihp, db_p, dw_hhp = ws[key]
    ops.tape_keep(dw_ihp, db_p, dw_hhp)

    def dw_ih():
        t, bm, bn, target = ops.tn_tile(2 * NP, E, cap)
        ops.gemm(dg, st['xd'], dw_ihp, M=2 * NP, N=E, K=cap, lda=2 * NP, ldb=E, ldc=E, trans_a=True, trans_b=True,
                 split_k=ops.split_for(2 * NP, E, cap, bm, bn, target), atomic=True, dyn=plan.total, dyn_dim=2, colsum_out=db_p, tile=t,
                 flop_scale=4.0 * H / NP)

    def dw_hh(d):
        t, bm, bn, target = ops.tn_tile(NP, H, cap, gather=True)
        ops.gemm(dg[:, d * NP:], st['hout'][:, d * H:], dw_hhp[d], M=NP, N=H, K=cap, lda=2 * NP, ldb=H2, ldc=H, trans_a=True,
                 trans_b=True, b_idx=(plan.prev_f, plan.prev_r)[d], split_k=ops.split_for(NP, H, cap, bm, bn, target), atomic=True,
                 dyn=plan.total, dyn_dim=2, tile=t, flop_scale=4.0 * H / NP)

    def table_hook():
        hook = mod.__dict__.get('_table_scatter_hook')       # data parallel: the table's gradient bucket goes out after the last scatter
        if hook is not None:
            hook(mod.__dict__.get('_table_scatters', 2))

    def dx_scatter():
        # d(embedding rows): dX = dgates . W_ihp (NT on the transposed packed weight), scattered into the table gradient through the
        # dropout mask.  Plain-store GEMM into the cell-state buffer (dead after the recurrence backward; xd / hout are still being read
        # by the weight-gradient GEMMs on the leaf stream) + the row-scatter kernel: the atomic epilogue of the fused form costs the GEMM
        # 18 % (764 vs 624 us alone, tools/dx_epilogue_bench.py; step 11.46 vs 11.51 ms)
        # (the cell buffer is [cap, 2*HP]: large enough only when 2*HP >= E -- not at --hidden_dim <= 144 with E = 300)
        dx = st['cell'].view(-1)[:cap * E].view(cap, E) if st['cell'].numel() >= cap * E else torch.empty((cap, E), **f32)
        ops.gemm(dg, w.w_ihp_t, dx, M=cap, N=E, K=2 * NP, lda=2 * NP, ldb=2 * NP, ldc=E, dyn=plan.total, dyn_dim=1, flop_scale=4.0 * H / NP)
        if st.get('tsort') is not None:
            ops.embed_scatter_sorted(dx, st['tsort'], grad_of(emb), p, st['seed'])
        else:
            ops.embed_scatter(dx, plan.tok, grad_of(emb), p, st['seed'], dyn=plan.total)

    # Data parallelism (world > 1), NNR_DP_TABLE_FIRST (opt-in: its benefit needs >= 2 GPUs to measure): the word-embedding table is 70 % of the
    # gradient bytes and its bucket can only leave after the LAST embedding-row scatter.  Both token streams then compute their
    # embedding-row gradient FIRST -- the weight-gradient GEMMs of the stream are issued behind the scatter instead of beside the dX
    # GEMM --, so the table bucket's all-reduce (72 MB: ~0.8 ms on one xGMI ring) starts ~2 ms before the end of the backward pass
    # and is hidden behind those GEMMs, instead of ~0.5 ms before it.  Single-GPU cost of this order: +0.05-0.1 ms.
    table_first = _DP_TABLE_FIRST == 1 or (_DP_TABLE_FIRST < 0 and mod.__dict__.get('_table_scatter_hook') is not None and _dp_world() > 1)
    if table_first:
        dx_scatter()
        table_hook()
        if leaf is None:
            dw_ih(); dw_hh(0); dw_hh(1)
        else:
            leaf(lambda: (dw_ih(), dw_hh(1)), dw_ihp, db_p, dw_hhp)         # (the leaf stream waits for this stream: behind the scatter)
            dw_hh(0)
            leaf.sync()
        ops.lstm_unpack_grads(dw_ihp, db_p, dw_hhp, H, E, [grad_of(q) for q in st['lstm'].param_list()], zero_src=True)
        return
    if leaf is None:
        # title streams (side stream, beside the content recurrence): the weight gradients, then the scatter GEMM (scatter first:
        # no gain either way, 12.39 vs 12.42-12.58 ms/step)
        dw_ih(); dw_hh(0); dw_hh(1)
        ops.lstm_unpack_grads(dw_ihp, db_p, dw_hhp, H, E, [grad_of(q) for q in st['lstm'].param_list()], zero_src=True)
        dx_scatter()
        table_hook()
        return
    # two balanced halves: leaf stream dW_ih + dW_hh(reverse), this stream the scatter GEMM + dW_hh(forward)
    leaf(lambda: (dw_ih(), dw_hh(1)), dw_ihp, db_p, dw_hhp)
    dx_scatter()
    table_hook()
    dw_hh(0)
    leaf.sync()
    ops.lstm_unpack_grads(dw_ihp, db_p, dw_hhp, H, E, [grad_of(q) for q in st['lstm'].param_list()], zero_src=True)


@torch.no_grad()
def cne_history_dedup(mod, title_text, title_mask, content_text, content_mask, category, subCategory):
    """SURVEY.md section 8 f-3, the EXACT part for CNE (inference, dropout off): every short history is right-padded with news 0
    (MIND_corpus.py:352-353,369) -- on MIND-shaped batches half of the 50 slots per user -- and userEncoders.py:76-78 runs the news
    encoder over all of them.  A PAD slot's representation depends only on its own (constant) inputs and on the two cell states that
    gate it (newsEncoders.py:128-129: the content at its title's sorted rank, the title at its content's sorted rank).  When both of
    those belong to PAD-like sequences too (one token, id 0 -- their cell states are one constant each), the slot's representation is
    THE constant r_pad.  Those slots are dropped from the encoder call, one representative computes r_pad, and every kept sequence
    keeps its original partner (a dropped partner is replaced by the representative: same cell state).  Decided on the device from
    the ranks; one host read of the kept count.  Returns (representations [B, H, D], number of sequences actually encoded)."""
    assert not mod.training or mod.dropout_rate == 0.0, 'de-duplication is exact only without dropout (one mask per slot otherwise)'
    B, Hn = title_text.shape[:2]
    n, T, Cx = B * Hn, mod.max_title_length, mod.max_content_length
    dev = title_text.device
    tm, cm = title_mask.view(n, T), content_mask.view(n, Cx)
    tm[:, 0] = 1                                        # in place on the caller's tensors, as every CNE call does (newsEncoders.py:108-109)
    cm[:, 0] = 1
    tt, ct = ops.ids32(title_text, n, T), ops.ids32(content_text, n, Cx)
    tlen, clen = tm.sum(dim=1), cm.sum(dim=1)
    order_t = torch.sort(tlen, descending=True, stable=True)[1]
    order_c = torch.sort(clen, descending=True, stable=True)[1]
    rank_t, rank_c = torch.empty_like(order_t), torch.empty_like(order_c)
    ar = torch.arange(n, device=dev)
    rank_t[order_t], rank_c[order_c] = ar, ar
    pc_t, pt_c = order_c[rank_t], order_t[rank_c]       # partner sequences under the call's own rank pairing
    cat, sub = ops.ids32(category, n), ops.ids32(subCategory, n)
    padlike = (tlen == 1) & (tt[:, 0] == 0) & (clen == 1) & (ct[:, 0] == 0) & (cat == 0) & (sub == 0)
    drop = padlike & padlike[pc_t] & padlike[pt_c]
    nd = int(drop.sum())
    if nd <= 1 or mod.tie_order != 'stable':
        rep, _ = cne_forward(mod, title_text, title_mask, content_text, content_mask, category, subCategory)
        return rep, n
    rep_idx = torch.nonzero(drop)[0, 0]                                  # the representative PAD slot
    keep = ~drop
    keep[rep_idx] = True
    kept = torch.nonzero(keep).flatten()                                 # original index of compact sequence k
    compact = torch.full((n,), -1, device=dev, dtype=torch.long)
    compact[kept] = torch.arange(kept.numel(), device=dev)
    rep_c = compact[rep_idx]
    remap = lambda partner: torch.where(compact[partner[kept]] >= 0, compact[partner[kept]], rep_c)
    sel = lambda x, w: x.reshape(n, w)[kept].unsqueeze(0).contiguous() if w else x.reshape(n)[kept].unsqueeze(0).contiguous()
    (out, _), = [(_cne_fwd_post(mod, sv, False)) for sv in [_cne_fwd_pre_and_lstm(mod, sel(tt, T), sel(tm, T), sel(ct, Cx), sel(cm, Cx),
                                                                                 sel(cat, 0), sel(sub, 0), (remap(pc_t), remap(pt_c)))]]
    D = out.shape[-1]
    full = out.view(-1, D)[rep_c].expand(n, D).clone()
    full[kept] = out.view(-1, D)
    return full.view(B, Hn, D), int(kept.numel())


def _cne_fwd_pre_and_lstm(mod, tt, tm, ct, cm, cat, sub, partner):
    sv = _cne_fwd_pre(mod, tt, tm, ct, cm, cat, sub, par=False, partner=partner)
    ops.lstm_fwd([sv['streams'][1], sv['streams'][0]], mod.hidden_dim)
    return sv


class CNE(NewsEncoder):
    """newsEncoders.py:57-141."""
    cne_streams, cne_gate, cne_cross = ('title', 'content'), True, True      # what the packed pipeline above runs for this class

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        self.max_title_length = config.max_title_length
        self.max_content_length = config.max_abstract_length
        self.hidden_dim = config.hidden_dim
        self.attention_dim = config.attention_dim
        self.news_embedding_dim = config.hidden_dim * 4 + config.category_embedding_dim + config.subCategory_embedding_dim
        self.tie_order = getattr(config, 'tie_order', 'stable')
        h2 = self.hidden_dim * 2
        self.title_lstm = LSTMParams(self.word_embedding_dim, self.hidden_dim)
        self.content_lstm = LSTMParams(self.word_embedding_dim, self.hidden_dim)
        self.title_H = nn.Linear(h2, h2, bias=False)
        self.title_M = nn.Linear(h2, h2, bias=True)
        self.content_H = nn.Linear(h2, h2, bias=False)
        self.content_M = nn.Linear(h2, h2, bias=True)
        self.title_self_attention = Attention(h2, config.attention_dim)
        self.content_self_attention = Attention(h2, config.attention_dim)
        self.title_cross_attention = ScaledDotProduct_CandidateAttention(h2, h2, config.attention_dim)
        self.content_cross_attention = ScaledDotProduct_CandidateAttention(h2, h2, config.attention_dim)

    def initialize(self):
        super().initialize()
        for lstm in (self.title_lstm, self.content_lstm):
            for parameter in lstm.parameters():
                if len(parameter.size()) >= 2:
                    nn.init.orthogonal_(parameter.data)
                else:
                    nn.init.zeros_(parameter.data)
        gain = nn.init.calculate_gain('sigmoid')
        for lin in (self.title_H, self.title_M, self.content_H, self.content_M):
            nn.init.xavier_uniform_(lin.weight, gain=gain)
        nn.init.zeros_(self.title_M.bias)
        nn.init.zeros_(self.content_M.bias)
        self.title_self_attention.initialize()
        self.content_self_attention.initialize()
        self.title_cross_attention.initialize()
        self.content_cross_attention.initialize()

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        # title_entity / content_entity / user_embedding are accepted and ignored, as in the reference (newsEncoders.py:102-141)
        return _CNEFunction.apply(self.word_embedding.weight, self, title_text, title_mask, content_text, content_mask, category, subCategory)

    def forward_pair(self, cand, hist):
        """(candidate call, history call) -> (candidate reps, history reps); same results as two forward() calls, with the
        two calls' Bi-LSTM recurrences sharing one launch.  cand / hist = (title_text, title_mask, content_text, content_mask,
        category, subCategory)."""
        return _CNEPairFunction.apply(self.word_embedding.weight, self, *cand, *hist)


class _CNEAblation(NewsEncoder):
    """The news-encoder ablations of the paper (variantEncoders.py:14-99,190-339): CNE with a stream, the cross-selective gate or the cross
    attention taken out.  A subclass names the streams it keeps and two flags; the packed CNE pipeline above runs what they describe, so an
    ablation issues a subset of CNE's launches.  Parameters are registered in the reference's order under the reference's names.

    tie_order is accepted by all four; without the gate nothing is paired by sorted rank, the order of equal lengths cannot reach a result
    and a representation depends on its own news only (batch_independent).  pad_dedup = False: Model.forward's inference de-duplication of
    PAD history slots (cne_history_dedup) is CNE's."""
    pad_dedup = False

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        self.max_title_length = config.max_title_length
        self.max_content_length = config.max_abstract_length
        self.hidden_dim = config.hidden_dim
        self.attention_dim = config.attention_dim
        h2 = self.hidden_dim * 2
        self.news_embedding_dim = h2 * len(self.cne_streams) + config.category_embedding_dim + config.subCategory_embedding_dim
        self.tie_order = getattr(config, 'tie_order', 'stable')
        for k in self.cne_streams:
            setattr(self, k + '_lstm', LSTMParams(self.word_embedding_dim, self.hidden_dim))
        for k in self.cne_streams if self.cne_gate else ():
            setattr(self, k + '_H', nn.Linear(h2, h2, bias=False))
            setattr(self, k + '_M', nn.Linear(h2, h2, bias=True))
        for k in self.cne_streams:
            setattr(self, k + '_self_attention', Attention(h2, config.attention_dim))
        for k in self.cne_streams if self.cne_cross else ():
            setattr(self, k + '_cross_attention', ScaledDotProduct_CandidateAttention(h2, h2, config.attention_dim))

    def initialize(self):
        super().initialize()
        for k in self.cne_streams:
            for parameter in getattr(self, k + '_lstm').parameters():
                if len(parameter.size()) >= 2:
                    nn.init.orthogonal_(parameter.data)
                else:
                    nn.init.zeros_(parameter.data)
        for k in self.cne_streams if self.cne_gate else ():
            nn.init.xavier_uniform_(getattr(self, k + '_H').weight)
            nn.init.xavier_uniform_(getattr(self, k + '_M').weight)
            nn.init.zeros_(getattr(self, k + '_M').bias)
        for k in self.cne_streams:
            getattr(self, k + '_self_attention').initialize()
        for k in self.cne_streams if self.cne_cross else ():
            getattr(self, k + '_cross_attention').initialize()

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        return _CNEFunction.apply(self.word_embedding.weight, self, title_text, title_mask, content_text, content_mask, category, subCategory)

    def forward_pair(self, cand, hist):
        """As CNE.forward_pair: the candidate call and the history call as one packed plan."""
        return _CNEPairFunction.apply(self.word_embedding.weight, self, *cand, *hist)


class CNE_Title(_CNEAblation):
    """variantEncoders.py:14-55: the title stream alone, Bi-LSTM rows -> self attention.  content_text / content_mask are never looked at."""
    cne_streams, cne_gate, cne_cross = ('title',), False, False
    batch_independent = True


class CNE_Content(_CNEAblation):
    """variantEncoders.py:58-99: the content stream alone; title_text / title_mask are never looked at."""
    cne_streams, cne_gate, cne_cross = ('content',), False, False
    batch_independent = True


class CNE_wo_CS(_CNEAblation):
    """variantEncoders.py:190-260, CNE without the cross-selective gate: both attentions read the raw Bi-LSTM rows; self + cross per stream."""
    cne_streams, cne_gate, cne_cross = ('title', 'content'), False, True
    batch_independent = True


class CNE_wo_CA(_CNEAblation):
    """variantEncoders.py:263-339, CNE without the cross attention: gated rows -> self attention, [title_self, content_self].  The gate pairs
    the two streams by sorted rank as CNE's does, so a representation depends on the other news of its call and on the tie order."""
    cne_streams, cne_gate, cne_cross = ('title', 'content'), True, False
    batch_independent = False


# ================================================================================================== MHSA / CNN
def mhsa_packed(enc, title_text):
    """MHSA news encoder over packed token rows (round 5).  Packed rows need the 4-head cooperative attention core (heads % 4 == 0,
    head_dim % 4 == 0, titles of at most 32 positions) and device tensors; anything else takes the dense path."""
    return (title_text.is_cuda and enc.head_num % 4 == 0 and enc.head_dim % 4 == 0 and enc.head_dim <= 32
            and enc.max_sentence_length <= 32 and enc.word_embedding_dim % 4 == 0)


class MHSA(NewsEncoder):
    """newsEncoders.py:173-200: title only; embedding gather -> QKV GEMMs -> MFMA attention core -> dropout ->
    additive attention pool -> feature fusion."""
    batch_independent = True          # a news representation does not depend on the other news of the call (evaluate.py cache)

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        self.max_sentence_length = config.max_title_length
        self.head_num, self.head_dim = config.head_num, config.head_dim
        self.feature_dim = config.head_num * config.head_dim
        self.multiheadAttention = MultiHeadAttention(config.head_num, config.word_embedding_dim, config.max_title_length,
                                                     config.max_title_length, config.head_dim, config.head_dim)
        self.attention = Attention(config.head_num * config.head_dim, config.attention_dim)
        self.news_embedding_dim = config.head_num * config.head_dim + config.category_embedding_dim + config.subCategory_embedding_dim

    def initialize(self):
        super().initialize()
        self.multiheadAttention.initialize()
        self.attention.initialize()

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        B, N = title_text.shape[:2]
        n, Lx = B * N, self.max_sentence_length
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        mask = title_mask.view(n, Lx)
        if mhsa_packed(self, title_text):
            # only the token rows that can reach the result (functional.MhsaPack): ~36 % of n * L at MIND title lengths
            pack = Fn.MhsaPack(mask, ops.ids32(title_text, n, Lx))
            w = Fn.PackedEmbedDropFn.apply(self.word_embedding.weight, pack, p, seed + 1)                   # [cap, E], live rows only
            qkv = Fn.QKVFn.apply(w, self.multiheadAttention, pack.plan.total)
            c = Fn.PackedMhsaCoreFn.apply(qkv, mask, pack, self.head_num, self.head_dim, p, seed + 2)       # [cap, h*d], dropout fused
            rep = Fn.PackedAttentionFn.apply(c, self.attention, mask, pack)                                 # [n, h*d]
            return Fn.FuseFn.apply(rep, self, category, subCategory, p, seed).view(B, N, self.news_embedding_dim)
        w = Fn.EmbedDropFn.apply(self.word_embedding.weight, title_text, p, seed + 1)                       # [n*L, E]
        qkv = Fn.QKVFn.apply(w, self.multiheadAttention, None)
        c = Fn.MhsaCoreFn.apply(qkv, mask, n, Lx, self.head_num, self.head_dim, p, seed + 2)                # [n*L, h*d], dropout fused
        rep = self.attention(c.view(n, Lx, self.feature_dim), mask)                                         # [n, h*d]
        return Fn.FuseFn.apply(rep, self, category, subCategory, p, seed).view(B, N, self.news_embedding_dim)


class CNN(NewsEncoder):
    """newsEncoders.py:144-170: title only; embedding gather -> Conv1d(k=3)+ReLU as shifted GEMMs -> dropout_ ->
    additive attention pool -> feature fusion."""
    batch_independent = True

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        self.max_sentence_length = config.max_title_length
        self.cnn_kernel_num = config.cnn_kernel_num
        self.conv = Conv1D(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size)
        self.attention = Attention(config.cnn_kernel_num, config.attention_dim)
        self.news_embedding_dim = config.cnn_kernel_num + config.category_embedding_dim + config.subCategory_embedding_dim

    def initialize(self):
        super().initialize()
        self.attention.initialize()

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        B, N = title_text.shape[:2]
        n, Lx = B * N, self.max_sentence_length
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        mask = title_mask.view(n, Lx)
        c = self.conv_text(title_text, self.conv.conv, n, Lx, p, seed)                                     # [n*L, C]
        rep = self.attention(c.view(n, Lx, self.cnn_kernel_num), mask)
        return Fn.FuseFn.apply(rep, self, category, subCategory, p, seed).view(B, N, self.news_embedding_dim)


class PNE(NewsEncoder):
    """newsEncoders.py:332-363, NPA's personalised news encoder: CNN's stages with the word-level pool replaced by a CandidateAttention whose
    query is relu(dense(user_embedding)) -- one additive attention per title with the query of a USER (csrc/pers_attn.hip: P exists for
    the B users, not for the B * news_num titles).

    Observable quirk kept: newsEncoders.py:359 builds the query rows with `.repeat([news_num, 1])`, so row r of the [B * news_num, ...] title
    list attends with user r % B -- not with the user r // news_num that owns it.  The two agree only when B == 1 or news_num == 1; with
    anything else a title is pooled with another sample's query, and evaluation scores depend on the batch size, as the reference's do.

    batch_independent is False: a representation depends on the user (and, through the quirk, on the batch), so evaluate.py does not cache."""
    batch_independent = False

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        self.max_sentence_length = config.max_title_length
        self.cnn_kernel_num = config.cnn_kernel_num
        self.personalized_embedding_dim = config.personalized_embedding_dim
        self.conv = Conv1D(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size)
        self.dense = nn.Linear(config.user_embedding_dim, config.personalized_embedding_dim, bias=True)
        self.personalizedAttention = CandidateAttention(config.cnn_kernel_num, config.personalized_embedding_dim, config.attention_dim)
        self.news_embedding_dim = config.cnn_kernel_num + config.category_embedding_dim + config.subCategory_embedding_dim

    def initialize(self):
        super().initialize()
        nn.init.xavier_uniform_(self.dense.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.dense.bias)
        self.personalizedAttention.initialize()

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        if user_embedding is None:
            raise Exception('PNE needs the user embedding rows (model.Model passes dropout(user_embedding(user_ID)))')
        B, N = title_text.shape[:2]
        n, Lx = B * N, self.max_sentence_length
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        mask = title_mask.view(n, Lx)
        c = self.conv_text(title_text, self.conv.conv, n, Lx, p, seed)                                     # [n*L, C]
        q_w = Fn.LinearFn.apply(user_embedding, self.dense.weight, self.dense.bias, ops.ACT_RELU, 0.0, 0)    # [B, personalized_embedding_dim]
        uidx = torch.arange(n, device=title_text.device, dtype=torch.int32) % B                            # the `.repeat` pairing: row r <- user r % B
        rep = personalized_attention(self.personalizedAttention, c.view(n, Lx, self.cnn_kernel_num), q_w, uidx, mask)
        return Fn.FuseFn.apply(rep, self, category, subCategory, p, seed).view(B, N, self.news_embedding_dim)


CONV1D_IMAGE = True         # the text stream's convolution as one padded-row product (functional.Conv1dImageFn); False (tools/naml_bench.py): CNN's shifted products


class _NAMLSingle(NewsEncoder):
    """variantEncoders.py:102-187, the single-view members of the NAML family over ONE text stream (`stream`: 'title' or 'content'):
    dropout(word rows) -> Conv1d + ReLU -> dropout_ -> additive attention pool over ALL positions -> multi-view attention with
    relu(category_affine(category row)) and relu(subCategory_affine(subCategory row)) (functional.ViewPoolFn, csrc/naml.hip).

    Observable quirks kept: no feature fusion (news_embedding_dim = cnn_kernel_num) and no mask -- PAD positions take part with row 0 of the
    word table, which is trainable like any other row; no dropout on the two category views; the masks, the entity arguments, the other
    text stream and `user_embedding` are accepted and ignored.  initialize() draws the three view-attention matrices with gain 1 and leaves
    the convolution as torch made it.  An even cnn_window_size gives the reference max_length - 1 convolution outputs: refused.
    Dropout seeds as CNN's: seed + 1 the word rows, seed + 2 the convolution output, both keyed on the compact (news, position, column)."""
    batch_independent = True

    def __init__(self, config, stream, word_table=None):
        super().__init__(config, word_table)
        if config.cnn_window_size % 2 == 0:
            raise Exception('cnn_window_size=%d: unsupported size (an even window leaves the reference one convolution output short of the '
                            'sequence length)' % config.cnn_window_size)
        self.text_stream = stream
        self.max_length = config.max_title_length if stream == 'title' else config.max_abstract_length
        setattr(self, 'max_%s_length' % stream, self.max_length)
        self.cnn_kernel_num = config.cnn_kernel_num
        self.news_embedding_dim = config.cnn_kernel_num
        setattr(self, stream + '_conv', Conv1D(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size))
        setattr(self, stream + '_attention', Attention(config.cnn_kernel_num, config.attention_dim))
        self.category_affine = nn.Linear(config.category_embedding_dim, config.cnn_kernel_num, bias=True)
        self.subCategory_affine = nn.Linear(config.subCategory_embedding_dim, config.cnn_kernel_num, bias=True)
        self.affine1 = nn.Linear(config.cnn_kernel_num, config.attention_dim, bias=True)
        self.affine2 = nn.Linear(config.attention_dim, 1, bias=False)

    def text_conv(self):
        return getattr(self, self.text_stream + '_conv')

    def text_attention(self):
        return getattr(self, self.text_stream + '_attention')

    def initialize(self):
        super().initialize()
        self.text_attention().initialize()
        for lin in (self.category_affine, self.subCategory_affine, self.affine1):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)
        nn.init.xavier_uniform_(self.affine2.weight)

    def text_view(self, text, n, p, seed):
        """One text stream's view [n, C]: the stages in front of the multi-view attention (a second stream is a second call of this)."""
        c = self.conv_text(text, self.text_conv().conv, n, self.max_length, p, seed, image=CONV1D_IMAGE)
        return self.text_attention()(c.view(n, self.max_length, self.cnn_kernel_num))                      # no mask

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        text = title_text if self.text_stream == 'title' else content_text
        B, N = text.shape[:2]
        n = B * N
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        view = self.text_view(text, n, p, seed)
        rep = Fn.ViewPoolFn.apply(self, category, subCategory, view)
        return rep.view(B, N, self.news_embedding_dim)


class NAML_Title(_NAMLSingle):
    """variantEncoders.py:102-143: the title stream (title_conv.*, title_attention.*)."""

    def __init__(self, config, word_table=None):
        super().__init__(config, 'title', word_table)


class NAML_Content(_NAMLSingle):
    """variantEncoders.py:146-187: the abstract stream, max_abstract_length positions (content_conv.*, content_attention.*)."""

    def __init__(self, config, word_table=None):
        super().__init__(config, 'content', word_table)


def _bow_streams(title_text, title_mask, content_text, content_mask):
    """ids [n, L] int32 and mask VIEWS [n, L] of both token streams of a call (views: an in-place mask fix must reach the caller's tensors)."""
    B, N, La = title_text.shape
    Lb = content_text.shape[2]
    n = B * N
    return (ops.ids32(title_text, n, La), title_mask.view(n, La), ops.ids32(content_text, n, Lb),
            content_mask.view(n, Lb))


class DAE(NewsEncoder):
    """newsEncoders.py:366-394, the denoising auto-encoder of the DAE-GRU baseline: m = sigmoid(mean of the word rows over the live positions
    of title and abstract together) (csrc/bag.hip, no [tokens, E] buffer), c = dropout(m), h = sigmoid(f1 c), d = sigmoid(f2 h);
    representation = feature_fusion(h).

    Observable quirks kept: the masks are not modified (a news without a live position is 0 / 0); `auxiliary_loss` = Alpha * ||m - d||_2,
    a [batch, news_num] device tensor that carries its own backward into m and d, is REWRITTEN by every call, in train and in eval mode.
    After Model.forward it is therefore the history call's [batch, max_history_num] tensor -- the candidate call's value is dropped and
    sends no gradient --, also when the candidate call runs on the side stream: that call is issued first, the history call last."""
    batch_independent = True

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        self.Alpha = config.Alpha
        assert self.Alpha > 0, 'Reconstruction loss weight must be greater than 0'
        self.f1 = nn.Linear(config.word_embedding_dim, config.hidden_dim, bias=True)
        self.f2 = nn.Linear(config.hidden_dim, config.word_embedding_dim, bias=True)
        self.news_embedding_dim = config.hidden_dim + config.category_embedding_dim + config.subCategory_embedding_dim

    def initialize(self):
        super().initialize()
        gain = nn.init.calculate_gain('sigmoid')
        for lin in (self.f1, self.f2):
            nn.init.xavier_uniform_(lin.weight, gain=gain)
            nn.init.zeros_(lin.bias)

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        B, N = title_text.shape[:2]
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        table = self.word_embedding.weight
        tt, tm, ct, cm = _bow_streams(title_text, title_mask, content_text, content_mask)
        m = Fn.BagMeanFn.apply(table, tt, tm, ct, cm, ops.ACT_SIGMOID, torch.is_grad_enabled() and table.requires_grad)    # [n, E]
        c = Fn.DropoutFn.apply(m, p, seed + 1) if p > 0 else m                                              # the corrupted embedding
        h = Fn.LinearFn.apply(c, self.f1.weight, self.f1.bias, ops.ACT_SIGMOID, 0.0, 0)                      # [n, hidden_dim]
        d = Fn.LinearFn.apply(h, self.f2.weight, self.f2.bias, ops.ACT_SIGMOID, 0.0, 0)                      # [n, E]
        self.auxiliary_loss = Fn.RowDistFn.apply(m, d, float(self.Alpha)).view(B, N)
        return Fn.FuseFn.apply(h, self, category, subCategory, p, seed).view(B, N, self.news_embedding_dim)


class Inception(NewsEncoder):
    """newsEncoders.py:397-433, the DFM baseline: title mean, abstract mean, category row and subCategory row side by side, a three-layer
    and a one-layer ReLU branch plus the plain sum of the four, and a linear layer over the three (functional.InceptionFn).  No dropout
    anywhere and no feature fusion.  Observable quirk kept: mask[:, :, 0] = 1 is set in place on the caller's title and abstract masks."""
    batch_independent = True

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        assert config.word_embedding_dim == config.category_embedding_dim and config.word_embedding_dim == config.subCategory_embedding_dim, \
            'embedding dimension must be the same in the Inception module'
        E = config.word_embedding_dim
        self.fc1_1 = nn.Linear(E * 4, config.hidden_dim, bias=True)
        self.fc1_2 = nn.Linear(config.hidden_dim, config.hidden_dim, bias=True)
        self.fc1_3 = nn.Linear(config.hidden_dim, E, bias=True)
        self.fc2 = nn.Linear(E * 4, E, bias=True)
        self.linear_transform = nn.Linear(E * 3, E, bias=True)
        self.news_embedding_dim = E

    def initialize(self):
        super().initialize()
        gain = nn.init.calculate_gain('relu')
        for lin in (self.fc1_1, self.fc1_2, self.fc1_3, self.fc2):
            nn.init.xavier_uniform_(lin.weight, gain=gain)
            nn.init.zeros_(lin.bias)
        nn.init.xavier_uniform_(self.linear_transform.weight)
        nn.init.zeros_(self.linear_transform.bias)

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        B, N = title_text.shape[:2]
        n = B * N
        table = self.word_embedding.weight
        tt, tm, ct, cm = _bow_streams(title_text, title_mask, content_text, content_mask)
        cat, sub = ops.ids32(category, n), ops.ids32(subCategory, n)
        rep = Fn.InceptionFn.apply(table, self, tt, tm, ct, cm, cat, sub, torch.is_grad_enabled() and table.requires_grad)
        return rep.view(B, N, self.news_embedding_dim)


class KCNN(NewsEncoder):
    """newsEncoders.py:203-241, the knowledge-aware CNN of the DKN baseline: per title position the word row, tanh(M_entity(entity row)) and
    tanh(M_context(context row)) as the three channels of an image, Conv2d(E -> cnn_kernel_num, kernel [cnn_window_size, 3]) over it, relu, the
    maximum over positions, feature fusion (functional.KcnnFn, csrc/kcnn.hip: one convolution product on the GEMM family).

    Observable quirks kept: no dropout before the fusion and no mask -- PAD positions take part with row 0 of each table, which is
    trainable like any other row; both knowledge tables are indexed by the same `title_entity` ids; the maximum runs over the first
    max_title_length - cnn_window_size + 1 convolution outputs only (layers.py:78).  `title_mask`, the content arguments and
    `user_embedding` are accepted and ignored.  initialize() leaves the knowledge tables and the convolution as they are."""
    batch_independent = True

    def __init__(self, config, word_table=None, entity_table=None, context_table=None):
        super().__init__(config, word_table)
        self.max_title_length = config.max_title_length
        self.cnn_kernel_num = config.cnn_kernel_num
        self.entity_embedding_dim = config.entity_embedding_dim
        self.context_embedding_dim = config.context_embedding_dim
        self.entity_embedding = nn.Embedding(num_embeddings=config.entity_size, embedding_dim=self.entity_embedding_dim)
        self.context_embedding = nn.Embedding(num_embeddings=config.entity_size, embedding_dim=self.context_embedding_dim)
        for emb, table, fname in ((self.entity_embedding, entity_table, 'entity_embedding-%s.pkl' % config.dataset),
                                  (self.context_embedding, context_table, 'context_embedding-%s.pkl' % config.dataset)):
            if table is None and os.path.exists(fname):              # the reference's behaviour (newsEncoders.py:212-215)
                with open(fname, 'rb') as f:
                    table = pickle.load(f)
            if table is not None:
                emb.weight.data.copy_(table)
        self.M_entity = nn.Linear(self.entity_embedding_dim, self.word_embedding_dim, bias=True)
        self.M_context = nn.Linear(self.context_embedding_dim, self.word_embedding_dim, bias=True)
        self.knowledge_cnn = Conv2D_Pool(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size, 3)
        self.news_embedding_dim = config.cnn_kernel_num + config.category_embedding_dim + config.subCategory_embedding_dim

    def initialize(self):
        super().initialize()
        gain = nn.init.calculate_gain('tanh')
        for lin in (self.M_entity, self.M_context):
            nn.init.xavier_uniform_(lin.weight, gain=gain)
            nn.init.zeros_(lin.bias)

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        B, N = title_text.shape[:2]
        n, Lx = B * N, self.max_title_length
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        table = self.word_embedding.weight
        text, entity = ops.ids32(title_text, n * Lx), ops.ids32(title_entity, n * Lx)
        rep = Fn.KcnnFn.apply(table, self, text, entity, n, Lx, torch.is_grad_enabled() and table.requires_grad)        # [n, C]
        return Fn.FuseFn.apply(rep, self, category, subCategory, p, seed).view(B, N, self.news_embedding_dim)


class HDC(NewsEncoder):
    """newsEncoders.py:244-278, the hierarchical dilated convolution of the FIM baseline: d0 = [category row | subCategory row | title word
    rows] (both category tables at width word_embedding_dim), three dilated Conv1d (dilations 1, 2, 3) each followed by LayerNorm([F, S]) and
    ReLU (functional.HdcFn, csrc/hdc.hip).  Only valid with the FIM user encoder and click predictor.

    The representation is the reference's pair (d0, dL), held position-major: d0 [B, N, S, E] and dL [3, B, N, S, F] where the reference has
    [B, N, E, S] and [B, N, 3, F, S] (S = max_title_length + 2); user_encoders.FIM reads this layout.  Observable quirks kept: no dropout and
    no mask -- PAD positions take part with row 0 of the word table, which is trainable like any other row; `news_embedding_dim` is None;
    the masks, the entity and content arguments and `user_embedding` are accepted and ignored.  The reference's padding (window - 1) // 2 +
    dilation - 1 keeps the sequence length only for HDC_window_size == 3 (its LayerNorm fails otherwise): other windows are refused."""

    def __init__(self, config, word_table=None):
        super().__init__(config, word_table)
        E, F, w = config.word_embedding_dim, config.HDC_filter_num, config.HDC_window_size
        if w != 3:
            raise Exception('HDC_window_size=%d: only 3 keeps the sequence length LayerNorm([HDC_filter_num, max_title_length + 2]) needs' % w)
        self.category_embedding = nn.Embedding(num_embeddings=config.category_num, embedding_dim=E)
        self.subCategory_embedding = nn.Embedding(num_embeddings=config.subCategory_num, embedding_dim=E)
        self.max_title_length = config.max_title_length
        self.HDC_sequence_length = config.max_title_length + 2
        self.HDC_filter_num = F
        self.dilated_conv1 = nn.Conv1d(in_channels=E, out_channels=F, kernel_size=w, padding=(w - 1) // 2, dilation=1)
        self.dilated_conv2 = nn.Conv1d(in_channels=F, out_channels=F, kernel_size=w, padding=(w - 1) // 2 + 1, dilation=2)
        self.dilated_conv3 = nn.Conv1d(in_channels=F, out_channels=F, kernel_size=w, padding=(w - 1) // 2 + 2, dilation=3)
        self.layer_norm1 = nn.LayerNorm([F, self.HDC_sequence_length])
        self.layer_norm2 = nn.LayerNorm([F, self.HDC_sequence_length])
        self.layer_norm3 = nn.LayerNorm([F, self.HDC_sequence_length])
        self.news_embedding_dim = None

    def dilated_convs(self):
        return (self.dilated_conv1, self.dilated_conv2, self.dilated_conv3)

    def layer_norms(self):
        return (self.layer_norm1, self.layer_norm2, self.layer_norm3)

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory, user_embedding):
        from . import functional as Fn
        B, N = title_text.shape[:2]
        n, Lx, S = B * N, self.max_title_length, self.HDC_sequence_length
        table = self.word_embedding.weight
        text = ops.ids32(title_text, n * Lx)
        cat, sub = ops.ids32(category, n), ops.ids32(subCategory, n)
        d0, dL = Fn.HdcFn.apply(table, self, text, cat, sub, n, Lx, torch.is_grad_enabled() and table.requires_grad)
        return d0.view(B, N, S, self.word_embedding_dim), dL.view(3, B, N, S, self.HDC_filter_num)
