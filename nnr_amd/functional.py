"""Autograd building blocks over the C-ABI for the MHSA / CNN / ATT encoders (dense [n, L, F] layouts).
Parameter gradients are accumulated straight into `param.grad` (see layers.grad_of); the Functions return gradients
only for activations."""
import math

import os
import torch

from . import ops
from .layers import attention_bwd, attention_fwd, grad_of


class EmbedDropFn(torch.autograd.Function):
    """dropout(word_embedding(ids))  -- nn.Embedding + in-place Dropout (newsEncoders.py:163,193)."""

    @staticmethod
    def forward(ctx, table, ids, p, seed):
        idx = ops.ids32(ids, -1)
        out = ops.embed_gather(table, idx, p, seed)
        ctx.table, ctx.idx, ctx.p, ctx.seed = table, idx, p, seed
        return out

    @staticmethod
    def backward(ctx, dout):
        ops.embed_scatter(dout.contiguous(), ctx.idx, grad_of(ctx.table), ctx.p, ctx.seed)
        return None, None, None, None


class UserRowsFn(torch.autograd.Function):
    """dropout(user_embedding(user_ID))  (model.py:122) for int64 ids [B]: the id is checked against the table size, and the backward sums
    duplicate ids in batch order without float atomics (csrc/misc.hip user_rows_*), so the table gradient is the same bits every run."""

    @staticmethod
    def forward(ctx, table, ids, p, seed):
        idx = ids.reshape(-1)
        idx = (idx if idx.dtype == torch.int64 else idx.to(torch.int64)).contiguous()
        out = ops.user_rows_fwd(table, idx, p, seed)
        ctx.table, ctx.idx, ctx.p, ctx.seed = table, idx, p, seed
        return out

    @staticmethod
    def backward(ctx, dout):
        ops.user_rows_bwd(dout.contiguous(), ctx.idx, grad_of(ctx.table), ctx.p, ctx.seed)
        return None, None, None, None


# ---------------------------------------------------------------------------------------------- MHSA news encoder over PACKED token rows
# (round 5)  The reference's MHSA news encoder multiplies all n * L padded positions through W_Q / W_K / W_V and the additive attention's
# affine1 (newsEncoders.py:187-200, layers.py:134-136,168); ~64 % of those rows are padding whose keys are masked (-1e9) and whose pooled
# weight is exactly 0.  Here only the rows ops.mask_cover names exist (every position up to a title's last valid one; ALL positions of a
# fully masked title, whose softmax is uniform), packed time-major by nnr_seq_plan exactly like CNE's token streams; the attention core
# finds position t of title i through a row map, the pool through the plan.  The original mask still masks keys and pooled positions.
class MhsaPack:
    """Plan + row map of one encoder call over `mask` [n, L] (bool / uint8) and `ids` [n, L] int32."""

    def __init__(self, mask, ids):
        cover = ops.mask_cover(mask)
        self.plan = ops.SeqPlan(cover, ids.contiguous(), None)          # (its in-place mask[:, 0] = 1 acts on `cover`: a no-op there)
        self.rowmap = ops.seq_rowmap(self.plan)
        self.cover = cover
        # round 6: two titles of <= 16 positions per 32 x 32 attention problem (the core's matrix work does not depend on a title's length)
        self.pair = ops.mhsa_pair_map(self.plan, mask) if self.plan.L == 32 else None


class PackedEmbedDropFn(torch.autograd.Function):
    """dropout(word_embedding(ids)) over the packed rows only; mask index = packed row * E + column."""

    @staticmethod
    def forward(ctx, table, pack, p, seed):
        plan = pack.plan
        out = ops.embed_gather(table, plan.tok, p, seed, dyn=plan.total)
        ctx.table, ctx.plan, ctx.p, ctx.seed = table, plan, p, seed
        return out

    @staticmethod
    def backward(ctx, dout):
        plan = ctx.plan
        ops.embed_scatter(dout.contiguous(), plan.tok, grad_of(ctx.table), ctx.p, ctx.seed, dyn=plan.total)
        return None, None, None, None


class PackedMhsaCoreFn(torch.autograd.Function):
    """MhsaCoreFn over packed rows: qkv / out are [cap, .] with only the plan's live rows defined."""

    @staticmethod
    def forward(ctx, qkv, mask, pack, heads, dh, p=0.0, seed=0):
        qkv = qkv.contiguous()
        out = torch.empty((pack.plan.cap, heads * dh), device=qkv.device, dtype=torch.float32)
        paired = pack.pair is not None and heads % 4 == 0 and dh % 4 == 0 and 32 * dh <= 768
        if paired:
            ops.mhsa_fwd_paired(qkv, pack.pair, pack.plan, heads, dh, out, p, seed)
        else:
            ops.mhsa_fwd_packed(qkv, mask, pack.rowmap, pack.plan, heads, dh, out, p, seed)
        ctx.qkv, ctx.mask, ctx.pack, ctx.dims, ctx.drop, ctx.paired = qkv, mask, pack, (heads, dh), (p, seed), paired
        return out

    @staticmethod
    def backward(ctx, dout):
        heads, dh = ctx.dims
        dqkv = torch.empty_like(ctx.qkv)
        if ctx.paired:
            ops.mhsa_bwd_paired(ctx.qkv, ctx.pack.pair, ctx.pack.plan, dout.contiguous(), heads, dh, dqkv, *ctx.drop)
        else:
            ops.mhsa_bwd_packed(ctx.qkv, ctx.mask, ctx.pack.rowmap, ctx.pack.plan, dout.contiguous(), heads, dh, dqkv, *ctx.drop)
        return dqkv, None, None, None, None, None, None


class PackedAttentionFn(torch.autograd.Function):
    """layers.py:167-175 over packed rows [cap, F]: tanh GEMM on the live rows, then the packed softmax pool (w2 . tanh(.) score inside the
    pool's pass, the ORIGINAL [n, L] mask applied to the scores); out [n, F] in the caller's row order."""

    @staticmethod
    def forward(ctx, feature, mod, mask, pack):
        plan = pack.plan
        cap, F = feature.shape
        A = mod.affine1.weight.shape[0]
        x = feature.contiguous()
        fused = A <= 256 and A % 4 == 0                               # the pool takes the w2 . th row-dot in its own pass
        th, score = attention_fwd(mod, x, dyn=plan.total, score=not fused)
        f32 = dict(device=x.device, dtype=torch.float32)
        alpha, out = torch.empty(cap, **f32), torch.empty((plan.n, F), **f32)
        sc = dict(th=th, w2=mod.affine2.weight) if fused else dict(score=score)
        ops.pool_fwd(x=x, ldx=F, D=F, n=plan.n, Lx=plan.L, plan=plan, mask=mask, alpha=alpha, out=out, ldo=F, **sc)
        ctx.mod, ctx.mask, ctx.plan, ctx.saved = mod, mask, plan, (x, th, alpha, F)
        return out

    @staticmethod
    def backward(ctx, dout):
        mod, plan = ctx.mod, ctx.plan
        x, th, alpha, F = ctx.saved
        f32 = dict(device=x.device, dtype=torch.float32)
        dx, ds = torch.empty((plan.cap, F), **f32), torch.empty(plan.cap, **f32)
        ops.pool_bwd(x=x, ldx=F, D=F, n=plan.n, Lx=plan.L, plan=plan, mask=ctx.mask, alpha=alpha, dout=dout.contiguous(), lddo=F, dx=dx, lddx=F, dscore=ds)
        attention_bwd(mod, x, th, ds, dx, plan)
        return dx, None, None, None


CAPTURE_RELU = [None]      # diagnostics / parity tests: set CAPTURE_RELU[0] = [] and every LinearFn with a ReLU appends its relu output r


class LinearFn(torch.autograd.Function):
    """y = dropout(act(x W^T + b)) for 2-D contiguous x;  act in {none, relu, tanh, sigmoid};  dropout mask keyed by the output element."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, p, seed):
        if act not in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH, ops.ACT_SIGMOID):
            raise ValueError('LinearFn: act must be none, relu, tanh or sigmoid')
        x = x.contiguous()
        M, K = x.shape
        N = weight.shape[0]
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
        # r = act(.) before the dropout, what the backward mask needs; behind a sigmoid or tanh without dropout y itself is that value
        smooth = act in (ops.ACT_SIGMOID, ops.ACT_TANH)
        r = torch.empty((M, N), device=x.device, dtype=torch.float32) if (act == ops.ACT_RELU or (smooth and p > 0)) else None
        ops.gemm(x, weight, y, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, act=act, aux_out=r, ldaux=N, drop=(3, p, seed, N))
        if CAPTURE_RELU[0] is not None and r is not None and act == ops.ACT_RELU:
            CAPTURE_RELU[0].append(r)
        if smooth and r is None:
            r = y.detach()               # (a second tensor object on y's storage: ctx must not hold its own output)
        ctx.x, ctx.weight, ctx.bias, ctx.r, ctx.act, ctx.p, ctx.seed = x, weight, bias, r, act, p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        if ctx.act == ops.ACT_SIGMOID:
            dz = torch.empty_like(dy)
            ops.sigmoid_drop_bwd(dy, ctx.r, dz, ctx.p, ctx.seed)
        elif ctx.act == ops.ACT_TANH:
            dz = torch.empty_like(dy)
            ops.tanh_drop_bwd(dy, ctx.r, dz, ctx.p, ctx.seed)
        elif ctx.act == ops.ACT_RELU or ctx.p > 0:
            dz = torch.empty_like(dy)
            r = ctx.r if ctx.r is not None else torch.ones_like(dy)
            ops.relu_drop_bwd(dy, r, dz, None, ctx.p, ctx.seed)
        else:
            dz = dy
        gw, gb, x = grad_of(ctx.weight), (grad_of(ctx.bias) if ctx.bias is not None else None), ctx.x
        ops.leaf_deferred(dz.device, dz.shape[0], lambda: ops.linear_bwd_weight(dz, x, gw, db=gb), dz, x)
        dx = ops.linear_bwd_data(dz, ctx.weight)
        return dx, None, None, None, None, None


class QKVFn(torch.autograd.Function):
    """[Q | K | V] = x W_{Q,K,V}^T + b  into one [M, 3*h*d] buffer (layers.py:134-136).  When the three weights sit back to
    back in the flat parameter buffer (trainer.FlatParams honours MultiHeadAttention.adjacent_parameter_groups) they ARE one
    [3*h*d, d_model] matrix: one GEMM forward, one K = 3*h*d GEMM for dX (no read-modify-write of dX), one for dW, one bias
    reduction.  Otherwise (module used on its own) the same three-GEMM sequence per projection."""

    @staticmethod
    def _stacked(mha, grads=False):
        from .layers import stacked_view
        ws, bs = (mha.W_Q.weight, mha.W_K.weight, mha.W_V.weight), (mha.W_Q.bias, mha.W_K.bias, mha.W_V.bias)
        if grads:
            ws, bs = [grad_of(w) for w in ws], [grad_of(b) for b in bs]
        w, b = stacked_view(ws), stacked_view(bs)
        return (w, b) if w is not None and b is not None else (None, None)

    @staticmethod
    def forward(ctx, x, mha, dyn=None):
        """dyn: device int32 with the number of LIVE rows of x (packed token rows: the rest of the buffer is undefined)."""
        x = x.contiguous()
        M, K = x.shape
        HD = mha.W_Q.weight.shape[0]
        qkv = torch.empty((M, 3 * HD), device=x.device, dtype=torch.float32)
        w, b = QKVFn._stacked(mha)
        dk = dict(dyn=dyn, dyn_dim=1) if dyn is not None else {}
        if w is not None:
            ops.gemm(x, w, qkv, M=M, N=3 * HD, K=K, lda=K, ldb=K, ldc=3 * HD, bias=b, **dk)
        else:
            for s, lin in enumerate((mha.W_Q, mha.W_K, mha.W_V)):
                ops.gemm(x, lin.weight, qkv[:, s * HD:], M=M, N=HD, K=K, lda=K, ldb=K, ldc=3 * HD, bias=lin.bias, **dk)
        ctx.x, ctx.mha, ctx.HD, ctx.dyn = x, mha, HD, dyn
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        dqkv = dqkv.contiguous()
        x, mha, HD, dyn = ctx.x, ctx.mha, ctx.HD, ctx.dyn
        M, K = x.shape
        dx = torch.empty_like(x)
        w, _ = QKVFn._stacked(mha)
        gw, gb = QKVFn._stacked(mha, grads=True) if w is not None else (None, None)
        d1 = dict(dyn=dyn, dyn_dim=1) if dyn is not None else {}        # live rows bound M of the data gradient ...
        d2 = dict(dyn=dyn, dyn_dim=2) if dyn is not None else {}        # ... and the reduction of the weight gradient
        if gw is not None:
            # dW (+ the bias gradient, fused into the same launch) is a leaf: own stream, joined at the end of the pass
            ops.leaf_deferred(x.device, M, lambda: ops.gemm(dqkv, x, gw, M=3 * HD, N=K, K=M, lda=3 * HD, ldb=K, ldc=K, trans_a=True,
                                                         trans_b=True, split_k=ops.split_for(3 * HD, K, M, *ops.tn_tile(3 * HD, K, M)[1:]), atomic=True,
                                                         colsum_out=gb, tile=ops.tn_tile(3 * HD, K, M)[0], **d2), dqkv, x)
            if M >= 1024 and w.is_contiguous():
                ops.gemm(dqkv, ops.wt(w), dx, M=M, N=K, K=3 * HD, lda=3 * HD, ldb=3 * HD, ldc=K, **d1)          # NT on [W_Q; W_K; W_V]^T
            else:
                ops.gemm(dqkv, w, dx, M=M, N=K, K=3 * HD, lda=3 * HD, ldb=K, ldc=K, trans_b=True, **d1)
            return dx, None, None
        for s, lin in enumerate((mha.W_Q, mha.W_K, mha.W_V)):
            d = dqkv[:, s * HD:]
            ops.gemm(d, lin.weight, dx, M=M, N=K, K=HD, lda=3 * HD, ldb=K, ldc=K, trans_b=True, accumulate=(s > 0), **d1)
            ops.gemm(d, x, grad_of(lin.weight), M=HD, N=K, K=M, lda=3 * HD, ldb=K, ldc=K, trans_a=True, trans_b=True,
                     split_k=ops.split_for(HD, K, M), atomic=True, **d2)
            ops.bias_grad(d, grad_of(lin.bias), rows=M, **({'dyn': dyn} if dyn is not None else {}))
        return dx, None, None


class MhsaCoreFn(torch.autograd.Function):
    """softmax(mask(Q K^T / sqrt(d_k))) V per head on the MFMA kernel (layers.py:137-147); p > 0 also applies the dropout
    that follows it (newsEncoders.py:196) in the kernel's output stage, same mask as DropoutFn(p, seed)."""

    @staticmethod
    def forward(ctx, qkv, mask, n, Lq, heads, dh, p=0.0, seed=0):
        qkv = qkv.contiguous()
        out = torch.empty((n * Lq, heads * dh), device=qkv.device, dtype=torch.float32)
        # the probabilities are not saved: backward recomputes them from Q, K (4 KB per head less HBM traffic each way)
        ops.mhsa_fwd(qkv, mask, n, Lq, heads, dh, out, None, p, seed)
        ctx.qkv, ctx.prob, ctx.mask, ctx.dims, ctx.drop = qkv, None, mask, (n, Lq, heads, dh), (p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, Lq, heads, dh = ctx.dims
        dqkv = torch.empty_like(ctx.qkv)
        ops.mhsa_bwd(ctx.qkv, ctx.mask, ctx.prob, dout.contiguous(), n, Lq, heads, dh, dqkv, *ctx.drop)
        return dqkv, None, None, None, None, None, None, None


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p, ctx.seed = p, seed
        return ops.dropout(x.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dy):
        return ops.dropout(dy.contiguous(), ctx.p, ctx.seed), None, None


class Conv1dReluFn(torch.autograd.Function):
    """relu(Conv1d(E -> C, kernel k, 'same' padding)) over [n, L, E] (layers.py:33-35) as k shifted GEMMs:
    y[(i,t), :] = sum_dt x[(i, t+dt), :] . W[:, :, dt]^T  (rows outside [0, L) read as zero through the row-gather index)."""

    @staticmethod
    def forward(ctx, x, conv, n, Lx):
        x = x.contiguous()
        E = x.shape[1]
        Cn, _, k = conv.weight.shape
        pad = (k - 1) // 2
        dev = x.device
        wt = torch.empty((k, Cn, E), device=dev, dtype=torch.float32)              # [k][C][E]  (Conv1d stores [C][E][k])
        ops.transpose2d(conv.weight, wt, Cn * E, k)
        t = torch.arange(Lx, device=dev, dtype=torch.int32)
        base = (torch.arange(n, device=dev, dtype=torch.int32) * Lx)[:, None]
        idxs = []
        for j in range(k):
            tt = t + (j - pad)
            idxs.append(torch.where((tt >= 0) & (tt < Lx), base + tt[None, :], torch.full_like(base + tt[None, :], -1)).reshape(-1).contiguous())
        M = n * Lx
        y = torch.empty((M, Cn), device=dev, dtype=torch.float32)
        for j in range(k):
            last = j == k - 1
            ops.gemm(x, wt[j], y, M=M, N=Cn, K=E, lda=E, ldb=E, ldc=Cn, a_idx=idxs[j], accumulate=(2 if j > 0 else 0),
                     bias=conv.bias if last else None, act=ops.ACT_RELU if last else 0)
        ctx.x, ctx.conv, ctx.wt, ctx.idxs, ctx.y, ctx.dims = x, conv, wt, idxs, y, (n, Lx, E, Cn, k)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, Lx, E, Cn, k = ctx.dims
        M = n * Lx
        dz = ops.relu_bwd(dy.contiguous(), ctx.y)
        dx = torch.zeros_like(ctx.x)
        x, idxs, gw, gb = ctx.x, ctx.idxs, grad_of(ctx.conv.weight), grad_of(ctx.conv.bias)

        def weight_grads():              # leaves (ops.leaf_deferred); the bias gradient rides on the first launch's A tiles
            dwt = torch.zeros_like(ctx.wt)
            for j in range(k):
                ops.gemm(dz, x, dwt[j], M=Cn, N=E, K=M, lda=Cn, ldb=E, ldc=E, trans_a=True, trans_b=True, b_idx=idxs[j],
                         split_k=ops.split_for(Cn, E, M), atomic=True, colsum_out=gb if j == 0 else None)
            ops.transpose2d(dwt, gw, k, Cn * E, accumulate=True)
        ops.leaf_deferred(dz.device, M, weight_grads, dz, x)
        for j in range(k):
            # dx[(i, t+dt)] += dz[(i,t)] . W_dt : scattered to the shifted row (a bijection on valid rows -> plain accumulate)
            ops.gemm(dz, ctx.wt[j], dx, M=M, N=E, K=Cn, lda=Cn, ldb=E, ldc=E, trans_b=True, c_idx=ctx.idxs[j], accumulate=True)
        return dx, None, None, None


class FuseFn(torch.autograd.Function):
    """feature_fusion (newsEncoders.py:50-54): [rep | dropout(category row) | dropout(subCategory row)]."""

    @staticmethod
    def forward(ctx, rep, enc, category, subCategory, p, seed):
        n, F = rep.shape
        cd, sd = enc.category_embedding.weight.shape[1], enc.subCategory_embedding.weight.shape[1]
        D = F + cd + sd
        out = torch.empty((n, D), device=rep.device, dtype=torch.float32)
        ops.add2d(out, D, rep.contiguous(), F, n, F)
        cat, sub = ops.ids32(category, n), ops.ids32(subCategory, n)
        # (both tables in one launch, the kernel of the CNE step; same per-element masks as two nnr_small_embed_fwd calls)
        ops.fusion_rows_fwd(enc.category_embedding.weight, enc.subCategory_embedding.weight, cat, sub, None, None, out[:, F:], D, p, seed + 3, seed + 4)
        ctx.enc, ctx.cat, ctx.sub, ctx.dims, ctx.p, ctx.seed = enc, cat, sub, (n, F, cd, sd, D), p, seed
        return out

    @staticmethod
    def backward(ctx, dout):
        n, F, cd, sd, D = ctx.dims
        dout = dout.contiguous()
        ops.fusion_rows_bwd(ctx.cat, ctx.sub, None, None, cd, sd, dout[:, F:], D, grad_of(ctx.enc.category_embedding.weight),
                            grad_of(ctx.enc.subCategory_embedding.weight), ctx.p, ctx.seed + 3, ctx.seed + 4)
        drep = torch.empty((n, F), device=dout.device, dtype=torch.float32)
        ops.add2d(drep, F, dout, D, n, F)
        return drep, None, None, None, None, None


class BagMeanFn(torch.autograd.Function):
    """act(masked mean of word-embedding rows over the live positions of the title and the abstract together) (newsEncoders.py:386-387,
    csrc/bag.hip): [n, E] from ids [n, La] / [n, Lb] int32 and masks [n, La] / [n, Lb]; the masks are not modified.  need_grad: the launch
    also writes the occurrence keys and their sort by word id runs on the leaf stream under the rest of the forward pass.  The table
    gradient is a reduction with one plain writer per row (no float atomics): always on the leaf stream, where the launches of the
    candidate call's and the history call's backward nodes cannot overlap."""

    @staticmethod
    def forward(ctx, table, ids_a, mask_a, ids_b, mask_b, act, need_grad):
        n, E = ids_a.shape[0], table.shape[1]
        dev = table.device
        out = torch.empty((n, E), device=dev, dtype=torch.float32)
        count = torch.empty(n, device=dev, dtype=torch.float32)
        plan = ops.BagPlan(n, ids_a.shape[1], ids_b.shape[1], table.shape[0], dev) if need_grad else None
        ops.bag_mean_fwd(table, ids_a, mask_a, ids_b, mask_b, False, act, out, E, 0, 0, count, plan)
        if plan is not None:
            plan.sort()
        ctx.table, ctx.saved, ctx.act = table, (out.detach(), count, plan), act
        return out

    @staticmethod
    def backward(ctx, dout):
        out, count, plan = ctx.saved
        ctx.saved = None
        dout = dout.contiguous()
        E, g, act = out.shape[1], grad_of(ctx.table), ctx.act
        ops.leaf_deferred(dout.device, 0, lambda: ops.bag_mean_bwd(dout, E, out, E, 0, 0, count, plan, False, act, g), dout, out, count, plan, force=True)
        return None, None, None, None, None, None, None


class RowDistFn(torch.autograd.Function):
    """coef * ||a[r] - b[r]||_2 per row of two [n, D] tensors (newsEncoders.py:391); zero gradient where the two rows are equal."""

    @staticmethod
    def forward(ctx, a, b, coef):
        a, b = a.contiguous(), b.contiguous()
        n = a.shape[0]
        dist = torch.empty(n, device=a.device, dtype=torch.float32)
        aux = torch.empty(n, device=a.device, dtype=torch.float32)
        ops.row_dist_fwd(a, b, coef, dist, aux)
        ctx.saved, ctx.coef = (a.detach(), b.detach(), dist), coef
        return aux

    @staticmethod
    def backward(ctx, gup):
        a, b, dist = ctx.saved
        da, db = torch.zeros_like(a), torch.zeros_like(b)
        ops.row_dist_bwd(a, b, dist, gup.contiguous().float(), ctx.coef, da, db)
        return da, db, None


class WbagFn(torch.autograd.Function):
    """The two weighted bags of DSSM (DSSM_model.py:29-30, csrc/dssm.hip) as one stacked [na + nb, E]: dropout(word_embedding(ids) * w).sum
    per row of the user stream `sa` and of the news stream `sb` (each (ids int32 [R, L], w f32 [R, L], sel int32 [n] or None)).  need_grad:
    the launch also writes the occurrence keys, and their sort by word id runs on the leaf stream under the towers.  The table gradient is
    a reduction with one plain writer per row over both streams' occurrences together (no float atomics)."""

    @staticmethod
    def forward(ctx, table, sa, sb, p, seed_a, seed_b, need_grad):
        dev, E = table.device, table.shape[1]
        na = sa[2].numel() if sa[2] is not None else sa[1].shape[0]
        nb = 0 if sb is None else (sb[2].numel() if sb[2] is not None else sb[1].shape[0])
        out = torch.empty((na + nb, E), device=dev, dtype=torch.float32)
        cap = na * sa[1].shape[1] + (nb * sb[1].shape[1] if sb is not None else 0)
        plan = ops.WbagPlan(cap, E, table.shape[0], dev) if need_grad else None
        ops.wbag_fwd(table, sa, sb, p, seed_a, seed_b, out, plan)
        if plan is not None:
            plan.sort()
        ctx.table, ctx.saved = table, (sa, sb, p, seed_a, seed_b, plan)
        return out

    @staticmethod
    def backward(ctx, dout):
        sa, sb, p, seed_a, seed_b, plan = ctx.saved
        ctx.saved = None
        ops.wbag_bwd(dout.contiguous(), sa, sb, p, seed_a, seed_b, plan, grad_of(ctx.table))
        return None, None, None, None, None, None, None


class CosineLossFn(torch.autograd.Function):
    """(logits [B, N], loss) of DSSM's cosine click head (DSSM_model.py:35-36, DSSM_main.py:63) from the stacked tower output y = [user rows
    [B, F] ; news rows [B * N, F]]: one launch computes both and d loss / d y, which the backward pass scales by the incoming gradient of
    the loss.  The logits are an output for the caller's eyes only (not differentiable on their own)."""

    @staticmethod
    def forward(ctx, y, B, N):
        y = y.contiguous()
        F, dev = y.shape[1], y.device
        logits = torch.empty((B, N), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        dlogits = torch.empty((B, N), device=dev, dtype=torch.float32)
        dy = torch.empty_like(y)
        ws = torch.empty(B, device=dev, dtype=torch.float32)
        ops.cosine_loss(y[:B], y[B:], B, N, F, logits, loss, dlogits, dy[:B], dy[B:], ws)
        ctx.saved = dy
        ctx.mark_non_differentiable(logits)
        return logits, loss

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        dy, ctx.saved = ctx.saved, None
        return dy * dloss, None, None


class InceptionFn(torch.autograd.Function):
    """The Inception news encoder (newsEncoders.py:421-433) for n news, forward and backward by hand so that the GEMMs' leading dimensions
    stand in for both torch.cat calls: emb [n, 4E] = [title mean | abstract mean | category row | subCategory row] (csrc/bag.hip in
    separate mode writes the first two slices, after setting mask[:, 0] = 1 in place), cat3 [n, 3E] = [relu(fc1_3 relu(fc1_2 relu(fc1_1
    emb))) | relu(fc2 emb) | sum of the four slices of emb], rep = linear_transform(cat3).  Parameter gradients go straight into .grad."""

    @staticmethod
    def forward(ctx, anchor, enc, tt, tm, ct, cm, cat, sub, need_grad):
        table = enc.word_embedding.weight
        n, E, dev = tt.shape[0], table.shape[1], table.device
        f32 = dict(device=dev, dtype=torch.float32)
        emb, count = torch.empty((n, 4 * E), **f32), torch.empty(2 * n, **f32)
        plan = ops.BagPlan(n, tt.shape[1], ct.shape[1], table.shape[0], dev) if need_grad else None
        ops.bag_mean_fwd(table, tt, tm, ct, cm, True, ops.ACT_NONE, emb, 4 * E, 0, E, count, plan)
        if plan is not None:
            plan.sort()
        ops.small_embed_fwd(enc.category_embedding.weight, cat, emb[:, 2 * E:], 4 * E, 0.0, 0)
        ops.small_embed_fwd(enc.subCategory_embedding.weight, sub, emb[:, 3 * E:], 4 * E, 0.0, 0)
        h1 = ops.linear_fwd(emb, enc.fc1_1.weight, enc.fc1_1.bias, act=ops.ACT_RELU)
        h2 = ops.linear_fwd(h1, enc.fc1_2.weight, enc.fc1_2.bias, act=ops.ACT_RELU)
        cat3 = torch.empty((n, 3 * E), **f32)
        ops.linear_fwd(h2, enc.fc1_3.weight, enc.fc1_3.bias, out=cat3[:, :E], act=ops.ACT_RELU)
        ops.linear_fwd(emb, enc.fc2.weight, enc.fc2.bias, out=cat3[:, E:2 * E], act=ops.ACT_RELU)
        s3 = cat3[:, 2 * E:]
        for k in range(4):                                            # ((title + abstract) + category) + subCategory, the reference's order
            ops.add2d(s3, 3 * E, emb[:, k * E:], 4 * E, n, E, accumulate=(k > 0))
        rep = ops.linear_fwd(cat3, enc.linear_transform.weight, enc.linear_transform.bias)
        ctx.enc, ctx.saved = enc, (emb, count, plan, h1, h2, cat3, cat, sub)
        return rep

    @staticmethod
    def backward(ctx, drep):
        enc = ctx.enc
        emb, count, plan, h1, h2, cat3, cat, sub = ctx.saved
        ctx.saved = None
        drep = drep.contiguous()
        n, E, dev = emb.shape[0], emb.shape[1] // 4, emb.device
        lt = enc.linear_transform
        wg = lambda dy, x, lin: ops.leaf_deferred(dev, n, lambda: ops.linear_bwd_weight(dy, x, grad_of(lin.weight), db=grad_of(lin.bias)), dy, x)
        wg(drep, cat3, lt)
        d1, d2, d3 = (ops.linear_bwd_data(drep, lt.weight[:, k * E:(k + 1) * E]) for k in range(3))     # the three column blocks of d cat3
        dz1 = ops.relu_bwd(d1, cat3[:, :E].contiguous())
        wg(dz1, h2, enc.fc1_3)
        dz_h2 = ops.relu_bwd(ops.linear_bwd_data(dz1, enc.fc1_3.weight), h2)
        wg(dz_h2, h1, enc.fc1_2)
        dz_h1 = ops.relu_bwd(ops.linear_bwd_data(dz_h2, enc.fc1_2.weight), h1)
        wg(dz_h1, emb, enc.fc1_1)
        demb = ops.linear_bwd_data(dz_h1, enc.fc1_1.weight)                                            # [n, 4E]
        dz2 = ops.relu_bwd(d2, cat3[:, E:2 * E].contiguous())
        wg(dz2, emb, enc.fc2)
        ops.linear_bwd_data(dz2, enc.fc2.weight, out=demb, accumulate=True)
        for k in range(4):
            ops.add2d(demb[:, k * E:], 4 * E, d3, E, n, E, accumulate=True)
        ops.small_embed_bwd(cat, E, demb[:, 2 * E:], 4 * E, grad_of(enc.category_embedding.weight), 0.0, 0)
        ops.small_embed_bwd(sub, E, demb[:, 3 * E:], 4 * E, grad_of(enc.subCategory_embedding.weight), 0.0, 0)
        g = grad_of(enc.word_embedding.weight)
        ops.leaf_deferred(dev, 0, lambda: ops.bag_mean_bwd(demb, 4 * E, None, 4 * E, 0, E, count, plan, True, ops.ACT_NONE, g), demb, count, plan,
                          force=True)
        return (None,) * 9


def rowconv_fwd(Xp, weight, out, **epilogue):
    """The convolution over a halo-padded row image as ONE product.  Xp [n (L + w - 1), Cin] has w - 1 zero halo rows
    per news, so row r of its overlapping-row view Xp' (lda = Cin < K = w Cin) is the window that starts at image row r:
    out[r] = epilogue(Xp'[r] . P^T) for every window inside the image, P the permuted weight; bias / act / c_idx go to the epilogue."""
    rows, Cin = Xp.shape
    Cn, w = weight.shape[0], weight.shape[2]
    ops.gemm(Xp, ops.rowconv_weight(weight, 0), out, M=rows - (w - 1), N=Cn, K=w * Cin, lda=Cin, ldb=w * Cin, ldc=Cn, **epilogue)


def rowconv_bwd(dzp, Xp, weight, leaf_rows, db=None):
    """Both gradients of rowconv_fwd from dzp [(w - 1) + n (L + w - 1), C]: the dense output gradient behind w - 1 leading zero rows, so row r
    of ITS overlapping-row view starts at dz row r - (w - 1).  Returns dXp = dz' . Q^T (Q: the transposed, window-reversed weight).  The
    weight gradient is one TN product over Xp' into a zeroed dP (db: the bias gradient, its column sums) that nnr_permute adds into
    weight.grad: a plain read-modify-write, so always on the ONE leaf stream, for both encoder calls."""
    rows, Cin = Xp.shape
    Cn, w = weight.shape[0], weight.shape[2]
    lead, R, gw = w - 1, rows - (w - 1), grad_of(weight)
    f32 = dict(device=Xp.device, dtype=torch.float32)

    def weight_grad():
        dP = torch.zeros((Cn, w * Cin), **f32)
        ops.linear_bwd_weight(dzp[lead:lead + R], Xp.as_strided((R, w * Cin), (Cin, 1)), dP, db=db)
        ops.permute(dP, gw, 'kcnn_dw', ops.rowconv_dims(weight), accumulate=True)
    ops.leaf_deferred(Xp.device, leaf_rows, weight_grad, dzp, Xp, force=True)
    dXp = torch.empty((rows, Cin), **f32)
    ops.gemm(dzp, ops.rowconv_weight(weight, 1), dXp, M=rows, N=Cin, K=w * Cn, lda=Cn, ldb=w * Cn, ldc=Cin)
    return dXp


class KcnnFn(torch.autograd.Function):
    """The KCNN news encoder up to its pooled [n, C] representation (newsEncoders.py:233-238, layers.py:77-78), forward and backward by hand
    around ONE convolution product (rowconv_fwd / rowconv_bwd; csrc/kcnn.hip):
      pre_j = table_j[entity] M_j^T + b_j (entity / context rows gathered in the GEMM's A loader);  Xp = the padded image [n, L + w - 1, 3 E]
      (word rows gathered straight from the table, tanh(pre_j), zero halo rows);  out = relu-then-max over the first L - w + 1 positions of
      the product + bias.  No dropout and no mask: PAD positions take part with row 0 of each table.  Backward: dense dz (every element
    written once), the two products, then the image apart again, the two projections' gradients with the table rows gathered in the B
    loader, and the three table gradients through the sorted scatter (reproducible, no pile-up of atomics on id 0).  Parameter gradients go
    straight into .grad."""

    @staticmethod
    def forward(ctx, anchor, enc, text, entity, n, Lx, need_grad):
        word, ent_t, ctx_t = enc.word_embedding.weight, enc.entity_embedding.weight, enc.context_embedding.weight
        conv = enc.knowledge_cnn.conv
        Cn, E, w, _ = conv.weight.shape
        dev, rows, Lp = word.device, n * Lx, Lx + w - 1
        f32 = dict(device=dev, dtype=torch.float32)
        sorts = None
        if need_grad:             # both sorts need nothing but the ids: on the leaf stream, under the forward pass
            sorts = (ops.TokenSort(text, None, word.shape[0]), ops.TokenSort(entity, None, ent_t.shape[0]))
        pre = []
        for tab, lin in ((ent_t, enc.M_entity), (ctx_t, enc.M_context)):
            D = tab.shape[1]
            y = torch.empty((rows, E), **f32)
            ops.gemm(tab, lin.weight, y, M=rows, N=E, K=D, lda=D, ldb=D, ldc=E, a_idx=entity, bias=lin.bias)
            pre.append(y)
        Xp = torch.empty((n * Lp, 3 * E), **f32)
        ops.kcnn_image_fwd(word, text, pre[0], pre[1], n, Lx, w, Xp)
        del pre
        z = torch.empty((n * Lp, Cn), **f32)                          # (its last w - 1 rows stay unwritten: no maximum reads them)
        rowconv_fwd(Xp, conv.weight, z)
        out = torch.empty((n, Cn), **f32)
        arg = torch.empty((n, Cn), device=dev, dtype=torch.uint8)
        ops.window_max_fwd(z, Cn, conv.bias, n, Cn, Lx, w, out, arg)
        ctx.enc, ctx.saved, ctx.dims = enc, (Xp if need_grad else None, arg, entity, sorts), (n, Lx, E, Cn, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        enc = ctx.enc
        Xp, arg, entity, (ts_word, ts_ent) = ctx.saved
        ctx.saved = None
        n, Lx, E, Cn, w = ctx.dims
        conv = enc.knowledge_cnn.conv
        dev, rows, Lp, lead = dout.device, n * Lx, Lx + w - 1, w - 1
        f32 = dict(device=dev, dtype=torch.float32)
        dout = dout.contiguous()
        dzp = torch.empty((lead + n * Lp, Cn), **f32)                 # w - 1 leading zero rows: row r of dz' starts at dz row r - (w - 1)
        db = torch.empty(Cn, **f32)
        ops.window_max_bwd(dout, arg, n, Cn, Lx, w, lead, dzp, db)
        gb = grad_of(conv.bias)
        ops.leaf_deferred(dev, rows, lambda: ops.add_(gb, db), db, force=True)        # (plain read-modify-write: one stream for both calls)
        dXp = rowconv_bwd(dzp, Xp, conv.weight, rows)
        dx0, dp1, dp2 = (torch.empty((rows, E), **f32) for _ in range(3))
        ops.kcnn_image_bwd(dXp, Xp, n, Lx, E, w, dx0, dp1, dp2)
        del dXp
        for tab, lin, dp in ((enc.entity_embedding.weight, enc.M_entity, dp1), (enc.context_embedding.weight, enc.M_context, dp2)):
            D = tab.shape[1]
            glw, glb = grad_of(lin.weight), grad_of(lin.bias)
            ops.leaf_deferred(dev, rows, lambda tab=tab, dp=dp, glw=glw, glb=glb, D=D: ops.gemm(
                dp, tab, glw, M=E, N=D, K=rows, lda=E, ldb=D, ldc=D, trans_a=True, trans_b=True, b_idx=entity, split_k=ops.split_for(E, D, rows),
                atomic=True, colsum_out=glb), dp, entity)
            ops.embed_scatter_sorted(ops.linear_bwd_data(dp, lin.weight), ts_ent, grad_of(tab), 0.0, 0)
        ops.embed_scatter_sorted(dx0, ts_word, grad_of(enc.word_embedding.weight), 0.0, 0)
        return (None,) * 7


class Conv1dImageFn(torch.autograd.Function):
    """relu(Conv1d(E -> C, window k odd, 'same' padding)) over dropout(word_table[text]) as ONE product (rowconv_fwd; csrc/naml.hip): the launch
    that gathers and drops the word rows writes them as the halo-padded image Xp [n, L + k - 1, E]; bias and relu sit in the product's
    epilogue, which writes the live rows compact through a row map: y [n L, C], as Conv1dReluFn's.  The word rows' keep-mask is
    nnr_embed_gather's for the same seed.  Backward: relu backward and the zero rows of the padded gradient in one launch, rowconv_bwd (the
    bias gradient rides on the weight gradient), and the word rows' gradient through the mask into the sorted scatter."""

    @staticmethod
    def forward(ctx, table, text, conv, n, Lx, p, seed, need_grad):
        E = table.shape[1]
        Cn, _, k = conv.weight.shape
        Lp, dev = Lx + k - 1, table.device
        idx = ops.ids32(text, -1)
        # the sort needs nothing but the ids: on the leaf stream, under the forward pass (the sorted scatter carries rows of <= 320 floats)
        ts = ops.TokenSort(idx, None, table.shape[0]) if need_grad and E <= 320 else None
        f32 = dict(device=dev, dtype=torch.float32)
        Xp = torch.empty((n * Lp, E), **f32)
        ops.conv1d_image_fwd(table, idx, n, Lx, k, p, seed, Xp)
        y = torch.empty((n * Lx, Cn), **f32)
        rowconv_fwd(Xp, conv.weight, y, bias=conv.bias, act=ops.ACT_RELU, c_idx=ops.conv1d_rowmap(n, Lx, k, dev))
        ctx.table, ctx.conv, ctx.saved, ctx.dims = table, conv, (Xp if need_grad else None, idx, ts, y), (n, Lx, E, Cn, k, p, seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        table, conv = ctx.table, ctx.conv
        Xp, idx, ts, y = ctx.saved
        ctx.saved = None
        n, Lx, E, Cn, k, p, seed = ctx.dims
        dev, Lp, lead = dy.device, Lx + k - 1, k - 1
        f32 = dict(device=dev, dtype=torch.float32)
        dzp = torch.empty((lead + n * Lp, Cn), **f32)                 # k - 1 leading zero rows: row r of the view starts at dz row r - (k - 1)
        ops.conv1d_dz_pad(dy.contiguous(), y, n, Lx, k, dzp)
        dXp = rowconv_bwd(dzp, Xp, conv.weight, n * Lx, db=grad_of(conv.bias))
        dx = torch.empty((n * Lx, E), **f32)
        ops.conv1d_image_bwd(dXp, n, Lx, k, p, seed, dx)
        if ts is not None:
            ops.embed_scatter_sorted(dx, ts, grad_of(table), 0.0, 0)
        else:
            ops.embed_scatter(dx, idx, grad_of(table), 0.0, 0)
        return (None,) * 8


class ViewPoolFn(torch.autograd.Function):
    """The multi-view attention of the NAML family (variantEncoders.py:137-142) over 1 or 2 text views [n, C] and the category and
    subCategory views (csrc/naml.hip): rep = sum_v softmax_v(affine2 . tanh(affine1(F_v))) * F_v.  The two table views are pure functions of
    an id (no dropout on them in the reference), so relu(affine(table)), its tanh projection and its score are computed once per TABLE row
    -- the text rows and the table rows go through affine1 as one [n Vt + Ra + Rb, C] operand -- and the kernel only indexes them; the
    [n, V, C] stack never exists.  Backward: the kernel sums the table rows' gradients over the news that name them in a fixed order, the
    rest are dense products over those n Vt + Ra + Rb rows; the embedding tables'
    gradients are [rows, dim] products, no scatter.  Parameter gradients go straight into .grad."""

    @staticmethod
    def forward(ctx, enc, category, subCategory, *texts):
        Vt, (n, Cn) = len(texts), texts[0].shape
        cat_t, sub_t = enc.category_embedding.weight, enc.subCategory_embedding.weight
        Ra, Rb = cat_t.shape[0], sub_t.shape[0]
        dev = texts[0].device
        f32 = dict(device=dev, dtype=torch.float32)
        cat, sub = ops.ids32(category, n), ops.ids32(subCategory, n)
        rows = n * Vt + Ra + Rb
        stack = torch.empty((rows, Cn), **f32)                      # [text view 0 | text view 1 | category rows | subCategory rows]
        for v, t in enumerate(texts):
            ops.add2d(stack[v * n:], Cn, t.contiguous(), Cn, n, Cn)
        rowsA, rowsB = stack[n * Vt:n * Vt + Ra], stack[n * Vt + Ra:]
        ops.linear_fwd(cat_t, enc.category_affine.weight, enc.category_affine.bias, out=rowsA, act=ops.ACT_RELU)
        ops.linear_fwd(sub_t, enc.subCategory_affine.weight, enc.subCategory_affine.bias, out=rowsB, act=ops.ACT_RELU)
        th, score = attention_fwd(enc, stack)
        alpha, out = torch.empty((n, Vt + 2), **f32), torch.empty((n, Cn), **f32)
        ops.view_pool_fwd([stack[v * n:(v + 1) * n] for v in range(Vt)], [score[v * n:(v + 1) * n] for v in range(Vt)], rowsA,
                          score[n * Vt:n * Vt + Ra], cat, rowsB, score[n * Vt + Ra:], sub, alpha, out)
        ctx.enc, ctx.saved, ctx.dims = enc, (stack, th, alpha, cat, sub), (Vt, n, Cn, Ra, Rb)
        return out

    @staticmethod
    def backward(ctx, dout):
        enc = ctx.enc
        stack, th, alpha, cat, sub = ctx.saved
        ctx.saved = None
        Vt, n, Cn, Ra, Rb = ctx.dims
        dev = dout.device
        f32 = dict(device=dev, dtype=torch.float32)
        dout = dout.contiguous()
        rows = n * Vt + Ra + Rb
        a0, b0 = n * Vt, n * Vt + Ra
        dstack, dscore = torch.empty((rows, Cn), **f32), torch.empty(rows, **f32)
        sl = lambda x: [x[v * n:(v + 1) * n] for v in range(Vt)]
        ops.view_pool_bwd(dout, sl(stack), stack[a0:b0], cat, stack[b0:], sub, alpha, sl(dstack), sl(dscore), dstack[a0:b0],
                          dscore[a0:b0], dstack[b0:], dscore[b0:])
        attention_bwd(enc, stack, th, dscore, dstack)
        dz_all = ops.relu_bwd(dstack[a0:], stack[a0:])                  # both tables' rows lie back to back: one launch
        for lo, hi, table, lin in ((0, Ra, enc.category_embedding.weight, enc.category_affine),
                                   (Ra, Ra + Rb, enc.subCategory_embedding.weight, enc.subCategory_affine)):
            dz, dim = dz_all[lo:hi], table.shape[1]
            ops.linear_bwd_weight(dz, table, grad_of(lin.weight), db=grad_of(lin.bias))
            # the table's gradient is a dense [rows, dim] product, added atomically: the candidate call's backward (side stream) and the
            # history call's (main stream) may overlap, and two addends into a zeroed buffer commute -- the same bits on every run
            ops.gemm(dz, lin.weight, grad_of(table), M=hi - lo, N=dim, K=Cn, lda=Cn, ldb=dim, ldc=dim, trans_b=True, atomic=True)
        return (None, None, None) + tuple(sl(dstack))


class ExpandFn(torch.autograd.Function):
    """[B, D] -> [B, N, D] (repeat / expand over the candidates, userEncoders.py:172,190); backward sums over N."""

    @staticmethod
    def forward(ctx, x, N):
        ctx.N = N
        return ops.expand_rows(x.contiguous(), N)

    @staticmethod
    def backward(ctx, dout):
        return ops.expand_rows_bwd(dout.contiguous()), None


class GruFn(torch.autograd.Function):
    """h_final [B, H] of nn.GRU over the first len[b] = mask[b].sum() slots of x [B, T, D] (csrc/gru.hip): the projection of every slot is one
    GEMM with the biases in its epilogue, the recurrence one launch.  h0 [B, H] or None (zeros); a user with len 0 returns h0[b] (or zero).
    Also returns len (int32 [B]) and hs [B, T, H] = h_t at every live slot, zero elsewhere (both not differentiable).  Backward: one recurrence
    launch that leaves the pre-activation gradients (zero at dead slots), then dX, the packed weight gradients and the bias sums as products /
    fixed-order column sums -- no float atomics."""

    @staticmethod
    def forward(ctx, x, mask, gru, h0):
        B, T, D = x.shape
        H = gru.hidden_dim
        x2 = x.contiguous().view(B * T, D)
        m8 = ops.mask_u8(mask)
        w = ops.gru_pack(gru, H, D)
        f32 = dict(device=x.device, dtype=torch.float32)
        gates = ops.linear_fwd(x2, w.w_ihp, w.b_p)                                               # [B*T, NP]
        hout, hprev = torch.zeros((B * T, H), **f32), torch.zeros((B * T, H), **f32)             # (dead slots stay zero)
        hfinal = torch.empty((B, H), **f32)
        length = torch.empty(B, device=x.device, dtype=torch.int32)
        h0c = h0.contiguous() if h0 is not None else None
        ops.gru_fwd(gates, m8, h0c, w, B, T, H, hout, hprev, hfinal, length)
        ctx.gru, ctx.saved, ctx.has_h0 = gru, (x2, gates, hprev, length, w, (B, T, D, H)), h0 is not None
        hs = hout.view(B, T, H)
        ctx.mark_non_differentiable(length, hs)
        return hfinal, length, hs

    @staticmethod
    def backward(ctx, dhfinal, _dlen, _dhs):
        gru = ctx.gru
        x2, gates, hprev, length, w, (B, T, D, H) = ctx.saved
        ctx.saved = None
        f32 = dict(device=x2.device, dtype=torch.float32)
        dh0 = torch.empty((B, H), **f32) if ctx.has_h0 else None
        ops.gru_bwd(gates, length, hprev, w, dhfinal.contiguous(), B, T, H, dh0)
        NP = w.NP
        dw_ihp, dw_hhp, db_p = torch.zeros((NP, D), **f32), torch.zeros((NP, H), **f32), torch.zeros(NP, **f32)
        for dw, act, K in ((dw_ihp, x2, D), (dw_hhp, hprev, H)):
            # reproducible: split-K only through the slab + fixed-order reduction (needs K % 4 == 0), never through float atomics
            split = ops.split_for(NP, K, B * T) if (K & 3) == 0 else 1
            ops.gemm(gates, act, dw, M=NP, N=K, K=B * T, lda=NP, ldb=K, ldc=K, trans_a=True, trans_b=True, atomic=split > 1, split_k=split)
        ops.bias_grad(gates, db_p)
        ops.gru_unpack_grads(dw_ihp, db_p, dw_hhp, H, D, [grad_of(t) for t in gru.param_list()])
        dx = ops.linear_bwd_data(gates, w.w_ihp)                                                  # zero at dead slots (slot 3 rows of w_ihp are zero)
        return dx.view(B, T, D), None, None, dh0


class GruDecFn(torch.autograd.Function):
    """tanh(h W^T + b) [B, D] with the rows of users without history (len[b] == 0) exactly zero, forward and backward (userEncoders.py:316-329:
    the reference concatenates zero rows, it does not decode a zero state)."""

    @staticmethod
    def forward(ctx, h, weight, bias, length):
        h = h.contiguous()
        y = ops.linear_fwd(h, weight, bias, act=ops.ACT_TANH)
        ops.gru_zero_empty(y, length)
        ctx.h, ctx.weight, ctx.bias, ctx.length, ctx.y = h, weight, bias, length, y.detach()
        return y

    @staticmethod
    def backward(ctx, dy):
        dz = torch.empty_like(ctx.y)
        ops.gru_tanh_bwd(dy.contiguous(), ctx.y, ctx.length, dz)
        ops.linear_bwd_weight(dz, ctx.h, grad_of(ctx.weight), db=grad_of(ctx.bias))
        return ops.linear_bwd_data(dz, ctx.weight), None, None, None


class HdcFn(torch.autograd.Function):
    """The HDC news encoder (newsEncoders.py:262-278) on position-major activations (csrc/hdc.hip): returns
    d0 [n, S, E] and dL [3, n, S, F] with S = max_title_length + 2.  Layer l (dilation d = l + 1, window 3, padding d) reads its input with d
    zero halo rows around every news, so its convolution is three accumulating products of the GEMM family on row pointers shifted by d rows;
    LayerNorm([F, S]) + ReLU writes the layer's output compact (what the matching images read) and halo-padded (what the next layer reads).
    Backward: per layer the gradient from the images and the one from the next layer are summed (images first), LayerNorm + ReLU backward
    runs in place on the saved convolution output, whose zeroed halo rows make the data gradient three accumulating products again; the three
    table gradients go through the sorted scatter.  Parameter gradients go straight into .grad."""

    @staticmethod
    def forward(ctx, anchor, enc, text, cat, sub, n, Lx, need_grad):
        word, cat_t, sub_t = enc.word_embedding.weight, enc.category_embedding.weight, enc.subCategory_embedding.weight
        convs, norms = enc.dilated_convs(), enc.layer_norms()
        E, Fn_, S = word.shape[1], enc.HDC_filter_num, Lx + 2
        dev = word.device
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        def padded(rows, C_):        # [rows, C]; one spare zero row behind it: the weight gradient reads rows of C rounded up to 4 columns
            buf = torch.empty((rows + 1, C_), **f32)
            ops.fill_zero(buf[rows:])
            return buf[:rows]
        d0, xp = torch.empty((n, S, E), **f32), padded(n * (S + 2), E)
        toks = torch.empty((3, n * S), **i32)
        ops.hdc_seq_fwd(word, cat_t, sub_t, text, cat, sub, n, Lx, 1, d0, xp, toks[0], toks[1], toks[2])
        sorts = None
        if need_grad:             # the sorts need nothing but the ids: on the leaf stream, under the forward pass
            sorts = tuple(ops.TokenSort(toks[j], None, t.shape[0]) for j, t in enumerate((word, cat_t, sub_t)))
        dL = torch.empty((3, n, S, Fn_), **f32)
        saved = []
        for l in range(3):
            d, Cin = l + 1, xp.shape[1]
            Sp = S + 2 * d
            M = n * Sp - 2 * d
            P = ops.hdc_weight(convs[l].weight)
            z = torch.empty((n * Sp, Fn_), **f32)
            for k in range(3):
                ops.gemm(xp[k * d:], P[k], z, M=M, N=Fn_, K=Cin, lda=Cin, ldb=Cin, ldc=Fn_, bias=convs[l].bias if k == 0 else None, accumulate=k > 0)
            stats = torch.empty((n, 2), **f32)
            nxt = padded(n * (S + 2 * (d + 1)), Fn_) if l < 2 else None
            ops.hdc_ln_relu_fwd(z, Sp, norms[l].weight, norms[l].bias, n, S, Fn_, norms[l].eps, dL[l], nxt, d + 1, stats)
            saved.append((xp, z, stats) if need_grad else None)
            xp = nxt
        ctx.enc, ctx.saved, ctx.dims = enc, (saved, sorts), (n, S, E, Fn_)
        ctx.save_for_backward(dL)          # (an output: held through autograd, not as an attribute, which would be a reference cycle)
        return d0, dL

    @staticmethod
    def backward(ctx, dd0, ddL):
        enc = ctx.enc
        saved, sorts = ctx.saved
        (dL,) = ctx.saved_tensors
        ctx.saved = None
        n, S, E, Fn_ = ctx.dims
        convs, norms = enc.dilated_convs(), enc.layer_norms()
        dev = ddL.device
        f32 = dict(device=dev, dtype=torch.float32)
        ddL = ddL.contiguous()
        dxp = None                                                    # gradient of layer l + 1's padded input
        for l in (2, 1, 0):
            d = l + 1
            Sp = S + 2 * d
            M = n * Sp - 2 * d
            xp, z, stats = saved[l]
            saved[l] = None
            Cin = xp.shape[1]
            dy = ddL[l]
            if dxp is not None:
                dy = torch.empty((n, S, Fn_), **f32)
                ops.hdc_unpad_add(ddL[l], dxp, n, S, d + 1, Fn_, dy)
            # the affine gradients of this call into a zeroed pair; added to .grad on the leaf stream (a plain read-modify-write: the candidate
            # call's backward runs on the side stream, the history call's on the main one, and the one leaf stream orders the two adds)
            dgb = ops.fill_zero(torch.empty((2,) + tuple(norms[l].weight.shape), **f32))
            ops.hdc_ln_relu_bwd(dy, dL[l], z, Sp, stats, norms[l].weight, n, S, Fn_, dgb[0], dgb[1])
            gg, gbeta = grad_of(norms[l].weight), grad_of(norms[l].bias)
            ops.leaf_deferred(dev, n * S, lambda dgb=dgb, gg=gg, gbeta=gbeta: (ops.add_(gg, dgb[0]), ops.add_(gbeta, dgb[1])), dgb, force=True)
            P = ops.hdc_weight(convs[l].weight)
            gw, gb = grad_of(convs[l].weight), grad_of(convs[l].bias)

            def weight_grad(xp=xp, z=z, d=d, M=M, Cin=Cin, gw=gw, gb=gb):
                # rows of Cin rounded up to 4 columns (the extra ones read the next row's head and are dropped): a column count that is a
                # multiple of 4 takes the split-K products through slabs and a fixed-order reduction, not through float atomics
                Cp = (Cin + 3) & ~3
                dP = torch.zeros((3, Fn_, Cp), **f32)
                for k in range(3):
                    ops.linear_bwd_weight(z[:M], xp[k * d:].as_strided((M, Cp), (Cin, 1)), dP[k], db=gb if k == 0 else None)
                ops.permute(dP, gw, 'hdc_dw', (Fn_, Cin, 3, Cp), accumulate=True)
            ops.leaf_deferred(dev, n * S, weight_grad, z, xp, force=True)
            dxp = ops.fill_zero(torch.empty((n * Sp, Cin), **f32))
            for k in range(3):
                ops.gemm(z, P[k], dxp[k * d:], M=M, N=Cin, K=Fn_, lda=Fn_, ldb=Cin, ldc=Cin, trans_b=True, accumulate=True)
        dx = torch.empty((n * S, E), **f32)
        ops.hdc_unpad_add(dd0.contiguous() if dd0 is not None else None, dxp, n, S, 1, E, dx)
        for ts, tab in zip(sorts, (enc.word_embedding.weight, enc.category_embedding.weight, enc.subCategory_embedding.weight)):
            ops.embed_scatter_sorted(dx, ts, grad_of(tab), 0.0, 0)
        return (None,) * 8


class FimFn(torch.autograd.Function):
    """The FIM user encoder (userEncoders.py:244-262): matching images -> two fused Conv3d + ELU + MaxPool3d layers (csrc/fim.hip) ->
    [B, N, feature_size] in the reference's flatten order.  cand_d0 [B N, S, E], cand_dL [3, B N, S, F], hist_d0 [B H, S, E], hist_dL
    [3, B H, S, F] (functional.HdcFn's layout).  The images are four batched products of the GEMM family (alpha = 1 / sqrt(F) for level 0
    too), one plane [B][N S][H S] per level: the first convolution layer reads them through its input strides, channel = level, depth =
    history slot, row = candidate position, column = history position.  Backward: the two layers' sparse backward passes, then eight
    batched products for the candidate- and history-side gradients of the four levels."""

    @staticmethod
    def forward(ctx, cand_d0, cand_dL, hist_d0, hist_dL, enc, B, N, H):
        S, Fn_ = cand_d0.shape[1], cand_dL.shape[3]
        cand_d0, cand_dL, hist_d0, hist_dL = cand_d0.contiguous(), cand_dL.contiguous(), hist_d0.contiguous(), hist_dL.contiguous()
        dev = cand_d0.device
        f32 = dict(device=dev, dtype=torch.float32)
        alpha = 1.0 / enc.scalar
        plane = B * N * S * H * S
        img = torch.empty((4, plane), **f32)
        levels = [(cand_d0, hist_d0)] + [(cand_dL[l], hist_dL[l]) for l in range(3)]
        for l, (c, h) in enumerate(levels):
            ops.match_images_fwd(c, h, B, N, H, S, alpha, img[l])
        ca, cb = enc.conv_3D_a, enc.conv_3D_b
        Ka, Kb, P, St = ca.kernel_size[0], cb.kernel_size[0], enc.pool_size, enc.pool_stride
        F1, F2, imgs = ca.out_channels, cb.out_channels, B * N
        strides_a = (S * H * S, plane, S, H * S, 1)
        da = ops.conv3d_pool_dims(4, H, S, S, F1, Ka, P, St)
        db = ops.conv3d_pool_dims(F1, da[0], da[1], da[2], F2, Kb, P, St)
        cells_a, cells_b = da[0] * da[1] * da[2], db[0] * db[1] * db[2]
        y1 = torch.empty((imgs, cells_a, F1), **f32)
        a1 = torch.empty((imgs, cells_a, F1), device=dev, dtype=torch.uint8)
        ops.conv3d_pool_fwd(img, strides_a, ops.conv3d_weight(ca.weight, 0), ca.bias, imgs, 4, H, S, S, F1, Ka, P, St, False, y1, a1)
        strides_b = (cells_a * F1, 1, da[1] * da[2] * F1, da[2] * F1, F1)
        y2 = torch.empty((imgs, F2 * cells_b), **f32)
        a2 = torch.empty((imgs, F2 * cells_b), device=dev, dtype=torch.uint8)
        ops.conv3d_pool_fwd(y1, strides_b, ops.conv3d_weight(cb.weight, 0), cb.bias, imgs, F1, da[0], da[1], da[2], F2, Kb, P, St, True, y2, a2)
        ctx.enc, ctx.saved = enc, (levels, img, y1, a1, y2, a2)
        ctx.dims = (B, N, H, S, Fn_, da, strides_a, strides_b)
        return y2.view(B, N, F2 * cells_b)

    @staticmethod
    def backward(ctx, dout):
        enc = ctx.enc
        levels, img, y1, a1, y2, a2 = ctx.saved
        ctx.saved = None
        B, N, H, S, Fn_, da, strides_a, strides_b = ctx.dims
        dev = dout.device
        f32 = dict(device=dev, dtype=torch.float32)
        ca, cb = enc.conv_3D_a, enc.conv_3D_b
        Ka, Kb, P, St = ca.kernel_size[0], cb.kernel_size[0], enc.pool_size, enc.pool_stride
        F1, F2, imgs = ca.out_channels, cb.out_channels, B * N
        dout = dout.contiguous()
        dy1 = torch.empty_like(y1)
        ops.conv3d_pool_bwd(dout, y2, a2, y1, strides_b, ops.conv3d_weight(cb.weight, 1), imgs, F1, da[0], da[1], da[2], F2, Kb, P, St, True, dy1,
                            grad_of(cb.weight), grad_of(cb.bias))
        dimg = torch.empty_like(img)
        ops.conv3d_pool_bwd(dy1, y1, a1, img, strides_a, ops.conv3d_weight(ca.weight, 1), imgs, 4, H, S, S, F1, Ka, P, St, False, dimg,
                            grad_of(ca.weight), grad_of(ca.bias))
        del img, dy1
        alpha = 1.0 / enc.scalar
        E = levels[0][0].shape[2]
        dc0, dh0 = torch.empty((B * N, S, E), **f32), torch.empty((B * H, S, E), **f32)
        dcL, dhL = torch.empty((3, B * N, S, Fn_), **f32), torch.empty((3, B * H, S, Fn_), **f32)
        for l, (c, h) in enumerate(levels):
            dc, dh = (dc0, dh0) if l == 0 else (dcL[l - 1], dhL[l - 1])
            ops.match_images_bwd(dimg[l], c, h, B, N, H, S, alpha, dc, dh)
        return dc0, dcL, dh0, dhL, None, None, None, None
