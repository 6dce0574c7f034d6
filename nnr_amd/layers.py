"""Layer classes of the hot path with the reference's names, constructor signatures and parameter names
(layers.py of the reference), so checkpoints / state_dicts are interchangeable.  Inside CNE / SUE the encoders drive
the HIP kernels directly from these parameter holders; the standalone `forward`s (dense [n, L, F] inputs, used by the
MHSA / ATT / CNN encoders) are autograd Functions over the same kernels."""
import math

import torch
import torch.nn as nn

from . import ops
from .ops import PARAM_EPOCH      # noqa: F401  (the derived-weight cache's epoch, importable here as before)


def grad_of(p):
    """`p.grad`, created zero-filled on first use.  The hand-written backward passes ACCUMULATE into it (the news
    encoder runs twice per step), exactly like autograd's AccumulateGrad; the trainer zeroes the flat gradient buffer."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def stacked_view(ts):
    """One [len(ts)*rows, ...] view over tensors that sit back to back in the same storage (see adjacent_parameter_groups),
    or None when they do not (a model that was not re-homed by the trainer: the callers then take the per-tensor path)."""
    t0 = ts[0]
    if not t0.is_contiguous():
        return None
    step = t0.numel()
    for i, t in enumerate(ts):
        if t.shape != t0.shape or not t.is_contiguous() or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr() \
                or t.storage_offset() != t0.storage_offset() + i * step:
            return None
    shape = (len(ts) * t0.shape[0],) + tuple(t0.shape[1:])
    stride = t0.stride()
    return t0.as_strided(shape, stride)


class LSTMParams(nn.Module):
    """Parameter holder with nn.LSTM(bidirectional=True, num_layers=1) names/shapes/default init (newsEncoders.py:66-67)."""

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        k = 1.0 / math.sqrt(hidden_dim)
        for sfx in ('', '_reverse'):
            for name, shape in (('weight_ih_l0', (4 * hidden_dim, input_dim)), ('weight_hh_l0', (4 * hidden_dim, hidden_dim)),
                                ('bias_ih_l0', (4 * hidden_dim,)), ('bias_hh_l0', (4 * hidden_dim,))):
                self.register_parameter(name + sfx, nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def param_list(self):
        return [self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0,
                self.weight_ih_l0_reverse, self.weight_hh_l0_reverse, self.bias_ih_l0_reverse, self.bias_hh_l0_reverse]


class GRUParams(nn.Module):
    """Parameter holder with nn.GRU(num_layers=1, batch_first=True) names/shapes/default init (userEncoders.py:290); gate order r | z | n."""

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        k = 1.0 / math.sqrt(hidden_dim)
        for name, shape in (('weight_ih_l0', (3 * hidden_dim, input_dim)), ('weight_hh_l0', (3 * hidden_dim, hidden_dim)),
                            ('bias_ih_l0', (3 * hidden_dim,)), ('bias_hh_l0', (3 * hidden_dim,))):
            self.register_parameter(name, nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def param_list(self):
        return [self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0]


# ------------------------------------------------------------------------------------------------ additive attention
def attention_fwd(mod, x, dyn=None, score=True):
    """th [rows, A] = tanh(affine1(x)) over a contiguous x [rows, F] and, with `score`, its row-dot with w2 [rows] (layers.py:167-169; without:
    the caller's pool takes th . w2 in its own pass).  dyn: device int32, the number of LIVE rows (packed rows: the rest is undefined)."""
    rows, F = x.shape
    A = mod.affine1.weight.shape[0]
    th = torch.empty((rows, A), device=x.device, dtype=torch.float32)
    dk = dict(dyn=dyn, dyn_dim=1) if dyn is not None else {}
    ops.gemm(x, mod.affine1.weight, th, M=rows, N=A, K=F, lda=F, ldb=F, ldc=A, bias=mod.affine1.bias, act=ops.ACT_TANH, **dk)
    s = torch.empty(rows, device=x.device, dtype=torch.float32) if score else None
    if score and A & 3:                  # nnr_rowdot reads a row four floats at a time: such an A as an N = 1 product
        ops.gemm(th, mod.affine2.weight, s, M=rows, N=1, K=A, lda=A, ldb=A, ldc=1, **dk)
    elif score:
        ops.rowdot(th, mod.affine2.weight, s, dyn=dyn)
    return th, s


def attention_bwd(mod, x, th, dscore, dx, plan=None):
    """The tail behind the pool's backward (which wrote dx and dscore): th := d(pre-activation) and dw2, the affine1 gradients as a leaf
    (own stream, ops.leaf_deferred), dx += th . W1.  plan: the packed rows' plan (live rows: plan.total)."""
    dyn = plan.total if plan is not None else None
    dk = dict(dyn=dyn, dyn_dim=1) if dyn is not None else {}
    ops.tanh_score_bwd(th, dscore, mod.affine2.weight, grad_of(mod.affine2.weight), plan, th.shape[1])
    gw, gb = grad_of(mod.affine1.weight), grad_of(mod.affine1.bias)
    ops.leaf_deferred(x.device, th.shape[0], lambda: ops.linear_bwd_weight(th, x, gw, db=gb, dyn=dyn), th, x)
    ops.linear_bwd_data(th, mod.affine1.weight, out=dx, accumulate=True, **dk)


class _AttentionFn(torch.autograd.Function):
    """layers.py:167-175 on a dense [n, L, F] feature: tanh GEMM, w2 row-dot, then the softmax pool."""

    @staticmethod
    def forward(ctx, feature, mod, mask):
        n, Lx, F = feature.shape
        x = feature.contiguous().view(n * Lx, F)
        th, score = attention_fwd(mod, x)
        f32 = dict(device=x.device, dtype=torch.float32)
        alpha, out = torch.empty(n * Lx, **f32), torch.empty((n, F), **f32)
        ops.pool_fwd(x=x, ldx=F, D=F, n=n, Lx=Lx, mask=mask, score=score, alpha=alpha, out=out, ldo=F)
        ctx.mod, ctx.mask, ctx.saved = mod, mask, (x, th, alpha, n, Lx, F)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, th, alpha, n, Lx, F = ctx.saved
        f32 = dict(device=x.device, dtype=torch.float32)
        dx, ds = torch.empty((n * Lx, F), **f32), torch.empty(n * Lx, **f32)
        ops.pool_bwd(x=x, ldx=F, D=F, n=n, Lx=Lx, mask=ctx.mask, alpha=alpha, dout=dout.contiguous(), lddo=F, dx=dx, lddx=F, dscore=ds)
        attention_bwd(ctx.mod, x, th, ds, dx)
        return dx.view(n, Lx, F), None, None


class Attention(nn.Module):
    """layers.py:151-175."""

    def __init__(self, feature_dim: int, attention_dim: int):
        super().__init__()
        self.affine1 = nn.Linear(feature_dim, attention_dim, bias=True)
        self.affine2 = nn.Linear(attention_dim, 1, bias=False)

    def initialize(self):
        nn.init.xavier_uniform_(self.affine1.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.affine1.bias)
        nn.init.xavier_uniform_(self.affine2.weight)

    def forward(self, feature, mask=None):
        return _AttentionFn.apply(feature, self, mask)


class ScaledDotProduct_CandidateAttention(nn.Module):
    """layers.py:178-203 (parameter holder; CNE and SUE evaluate it in its GEMV form, see their pipelines)."""

    def __init__(self, feature_dim: int, query_dim: int, attention_dim: int):
        super().__init__()
        self.K = nn.Linear(feature_dim, attention_dim, bias=False)
        self.Q = nn.Linear(query_dim, attention_dim, bias=True)
        self.attention_scalar = math.sqrt(float(attention_dim))

    def initialize(self):
        nn.init.xavier_uniform_(self.K.weight)
        nn.init.xavier_uniform_(self.Q.weight)
        nn.init.zeros_(self.Q.bias)

    def forward(self, feature, query, mask=None):
        """layers.py:196-203 on its own: feature [n, L, F], query [n, Qd], mask [n, L] -> [n, F].  GEMV form: the score of
        position t is <feature_t, K^T (Q query + b)> / sqrt(A), so K is never applied to the L x F features."""
        return _CandidateAttentionFn.apply(feature, query, self, mask)


class _CandidateAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feature, query, mod, mask):
        n, Lx, F = feature.shape
        A = mod.K.weight.shape[0]
        x = feature.contiguous().view(n * Lx, F)
        q = query.contiguous()
        f32 = dict(device=x.device, dtype=torch.float32)
        qv = ops.linear_fwd(q, mod.Q.weight, mod.Q.bias)                                       # [n, A]
        v = torch.empty((n, F), **f32)
        ops.gemm(qv, mod.K.weight, v, M=n, N=F, K=A, lda=A, ldb=F, ldc=F, trans_b=True)         # K^T (Q q + b)
        alpha = torch.empty(n * Lx, **f32)
        out = torch.empty((n, F), **f32)
        ops.pool_fwd(x=x, ldx=F, D=F, n=n, Lx=Lx, mask=mask, v=v, ldv=F, scale=1.0 / math.sqrt(A), alpha=alpha, out=out, ldo=F)
        ctx.mod, ctx.mask, ctx.saved = mod, mask, (x, q, qv, v, alpha, n, Lx, F, A)
        return out

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        x, q, qv, v, alpha, n, Lx, F, A = ctx.saved
        f32 = dict(device=x.device, dtype=torch.float32)
        dx = torch.empty((n * Lx, F), **f32)
        dv = torch.empty((n, F), **f32)
        ops.pool_bwd(x=x, ldx=F, D=F, n=n, Lx=Lx, mask=ctx.mask, v=v, ldv=F, scale=1.0 / math.sqrt(A), alpha=alpha, dout=dout.contiguous(),
                     lddo=F, dx=dx, lddx=F, dv=dv, lddv=F)
        dqv = torch.empty((n, A), **f32)
        ops.gemm(dv, mod.K.weight, dqv, M=n, N=A, K=F, lda=F, ldb=F, ldc=A)                     # dqv = dv . K^T
        ops.linear_bwd_weight(qv, dv, grad_of(mod.K.weight))                                    # dK[A, F] += qv^T dv
        ops.linear_bwd_weight(dqv, q, grad_of(mod.Q.weight))
        ops.bias_grad(dqv, grad_of(mod.Q.bias))
        dq = ops.linear_bwd_data(dqv, mod.Q.weight)
        return dx.view(n, Lx, F), dq, None, None


# ------------------------------------------------------------------------------------------------ candidate-aware additive attention
class _CandAttnFn(torch.autograd.Function):
    """alpha[b,n,:] = softmax_h(w2 . act(Wq query[b,n] + bq + Wf feature[b,h])), out[b,n] = alpha[b,n] . feature[b]: two projection GEMMs and the
    fused kernel of csrc/cand_attn.hip (the [B, N, H, A] hidden tensor of the reference is never stored; the backward pass recomputes the
    activations).  feature [B, H, F], query [B, N, Qd], mask [B, H] or None -> [B, N, F].  `mod` supplies the weights through
    _cand_attn_weights() -> (Wq [A, Qd], bq, Wf [A, F], w2 [A], act) and their gradient buffers through _cand_attn_grads() in the same order
    (row-strided views are fine: CATT's Wq | Wf are the two halves of ONE Linear(2D, A))."""

    @staticmethod
    def forward(ctx, feature, query, mod, mask):
        B, H, F = feature.shape
        N, Qd = query.shape[1], query.shape[2]
        wq, bq, wf, w2, act = mod._cand_attn_weights()
        A = w2.numel()
        x = feature.contiguous()
        q = query.contiguous().view(B * N, Qd)
        mask = ops.mask_u8(mask)
        f32 = dict(device=x.device, dtype=torch.float32)
        P = ops.linear_fwd(q, wq, bq)                                                           # [B*N, A]
        Q = ops.linear_fwd(x.view(B * H, F), wf)                                                # [B*H, A]
        alpha = torch.empty((B, N, H), **f32)
        out = torch.empty((B, N, F), **f32)
        ops.cand_attn_fwd(P, Q, w2, x, mask, B, N, H, A, F, act, alpha, out)
        ctx.mod, ctx.saved = mod, (x, q, P, Q, alpha, mask, (B, N, H, A, F, Qd))
        return out

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        x, q, P, Q, alpha, mask, (B, N, H, A, F, Qd) = ctx.saved
        ctx.saved = None
        wq, _, wf, w2, act = mod._cand_attn_weights()
        gwq, gbq, gwf, gw2 = mod._cand_attn_grads()
        f32 = dict(device=x.device, dtype=torch.float32)
        dP = torch.empty((B * N, A), **f32)
        dQ = torch.empty((B * H, A), **f32)
        dx = torch.empty((B, H, F), **f32)
        ops.cand_attn_bwd(P, Q, w2, x, mask, alpha, dout.contiguous(), B, N, H, A, F, act, dP, dQ, dx, gw2)
        ops.linear_bwd_data(dQ, wf, out=dx.view(B * H, F), accumulate=True)                      # the feature's share through Wf
        dq = ops.linear_bwd_data(dP, wq)
        ops.linear_bwd_weight(dP, q, gwq)
        ops.bias_grad(dP, gbq)
        ops.linear_bwd_weight(dQ, x.view(B * H, F), gwf)
        return dx, dq.view(B, N, Qd), None, None


class _PersAttnUnsupported(Exception):
    pass


class _PersAttnFn(torch.autograd.Function):
    """layers.CandidateAttention with the query taken through an index map: feature [n, L, F], query [U, Qd], uidx int32 [n] (title i attends
    with query uidx[i]), mask [n, L] or None -> [n, F], on csrc/pers_attn.hip.  The query projection and its gradient exist for U rows, not n;
    the [n, L, A] hidden tensor is never stored (the backward pass recomputes the activations).  `mod` supplies weights and gradient buffers
    as for _CandAttnFn (tanh only).  Raises _PersAttnUnsupported, before anything is computed, for a shape the kernel does not take:
    personalized_attention() then runs _CandAttnFn on the expanded query rows."""

    @staticmethod
    def forward(ctx, feature, query, uidx, mod, mask):
        n, Lx, F = feature.shape
        U, Qd = query.shape
        wq, bq, wf, w2, act = mod._cand_attn_weights()
        assert act == ops.ACT_TANH
        A = w2.numel()
        x = feature.contiguous()
        q = query.contiguous()
        uidx = ops.ids32(uidx, -1)
        mask = ops.mask_u8(mask)
        f32 = dict(device=x.device, dtype=torch.float32)
        P = ops.linear_fwd(q, wq, bq)                                                           # [U, A]
        Qf = ops.linear_fwd(x.view(n * Lx, F), wf)                                              # [n*L, A]
        alpha = torch.empty((n, Lx), **f32)
        out = torch.empty((n, F), **f32)
        if ops.pers_attn_fwd(Qf, P, uidx, w2, x, mask, n, Lx, A, F, alpha, out) != 0:
            raise _PersAttnUnsupported()
        ctx.mod, ctx.saved = mod, (x, q, uidx, P, Qf, alpha, mask, (n, Lx, A, F, U, Qd))
        return out

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        x, q, uidx, P, Qf, alpha, mask, (n, Lx, A, F, U, Qd) = ctx.saved
        ctx.saved = None
        wq, _, wf, w2, _ = mod._cand_attn_weights()
        gwq, gbq, gwf, gw2 = mod._cand_attn_grads()
        f32 = dict(device=x.device, dtype=torch.float32)
        dP = torch.empty((U, A), **f32)
        dQf = torch.empty((n * Lx, A), **f32)
        dx = torch.empty((n, Lx, F), **f32)
        ops.pers_attn_bwd(Qf, P, uidx, w2, x, mask, alpha, dout.contiguous(), n, Lx, A, F, dP, dQf, dx, gw2)
        ops.linear_bwd_data(dQf, wf, out=dx.view(n * Lx, F), accumulate=True)                   # the feature's share through Wf
        dq = ops.linear_bwd_data(dP, wq)
        ops.linear_bwd_weight(dP, q, gwq)
        ops.bias_grad(dP, gbq)
        ops.leaf_deferred(x.device, n * Lx, lambda: ops.linear_bwd_weight(dQf, x.view(n * Lx, F), gwf), dQf, x)
        return dx, dq, None, None, None


def personalized_attention(mod, feature, query, uidx, mask=None):
    """`mod` (a CandidateAttention) over feature [n, L, F] with title i's query = query[uidx[i]] (query [U, Qd], every uidx in [0, U)):
    the per-title kernel, or -- for a shape it returns NNR_ERR_UNSUPPORTED for -- the candidate-attention kernels on the expanded rows."""
    try:
        return _PersAttnFn.apply(feature, query, uidx, mod, mask)
    except _PersAttnUnsupported:
        return _CandAttnFn.apply(feature, query.index_select(0, uidx.long()).unsqueeze(dim=1), mod, mask).squeeze(dim=1)


class CandidateAttention(nn.Module):
    """layers.py:206-232: additive attention over `feature` with ONE query per sample (tanh)."""

    def __init__(self, feature_dim: int, query_dim: int, attention_dim: int):
        super().__init__()
        self.feature_affine = nn.Linear(feature_dim, attention_dim, bias=False)
        self.query_affine = nn.Linear(query_dim, attention_dim, bias=True)
        self.attention_affine = nn.Linear(attention_dim, 1, bias=False)

    def initialize(self):
        nn.init.xavier_uniform_(self.feature_affine.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.xavier_uniform_(self.query_affine.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.query_affine.bias)
        nn.init.xavier_uniform_(self.attention_affine.weight)

    def _cand_attn_weights(self):
        return self.query_affine.weight, self.query_affine.bias, self.feature_affine.weight, self.attention_affine.weight.view(-1), ops.ACT_TANH

    def _cand_attn_grads(self):
        return (grad_of(self.query_affine.weight), grad_of(self.query_affine.bias), grad_of(self.feature_affine.weight),
                grad_of(self.attention_affine.weight).view(-1))

    def forward(self, feature, query, mask=None):
        """feature [n, L, F], query [n, Qd], mask [n, L] -> [n, F]"""
        return _CandAttnFn.apply(feature, query.unsqueeze(dim=1), self, mask).squeeze(dim=1)


class MultipleCandidateAttention(CandidateAttention):
    """layers.py:235-262: the same with several queries per sample."""

    def forward(self, feature, query, mask=None):
        """feature [n, L, F], query [n, Nq, Qd], mask [n, L] -> [n, Nq, F]"""
        return _CandAttnFn.apply(feature, query, self, mask)


class MultiHeadAttention(nn.Module):
    """layers.py:102-148 (parameter holder + forward over the MFMA attention kernel, see news_encoders.MHSA)."""

    def __init__(self, h: int, d_model: int, len_q: int, len_k: int, d_k: int, d_v: int):
        super().__init__()
        self.h, self.d_model, self.len_q, self.len_k, self.d_k, self.d_v = h, d_model, len_q, len_k, d_k, d_v
        self.out_dim = h * d_v
        self.attention_scalar = math.sqrt(float(d_k))
        self.W_Q = nn.Linear(d_model, h * d_k, bias=True)
        self.W_K = nn.Linear(d_model, h * d_k, bias=True)
        self.W_V = nn.Linear(d_model, h * d_v, bias=True)

    def initialize(self):
        nn.init.xavier_uniform_(self.W_Q.weight)
        nn.init.zeros_(self.W_Q.bias)
        nn.init.xavier_uniform_(self.W_K.weight)
        nn.init.zeros_(self.W_K.bias)
        nn.init.xavier_uniform_(self.W_V.weight)
        nn.init.zeros_(self.W_V.bias)

    def adjacent_parameter_groups(self):
        """Parameters the flat buffer (trainer.FlatParams) should lay out back to back, in this order: the three projection
        weights then form ONE [3*h*d, d_model] matrix (and the biases one vector) without any copy, and functional.QKVFn runs
        one GEMM per direction instead of three.  Names, shapes and the state_dict stay the reference's."""
        if self.W_Q.weight.shape != self.W_K.weight.shape or self.W_Q.weight.shape != self.W_V.weight.shape:
            return []
        return [[self.W_Q.weight, self.W_K.weight, self.W_V.weight], [self.W_Q.bias, self.W_K.bias, self.W_V.bias]]


class Conv1D(nn.Module):
    """layers.py:7-44, 'naive' branch (the only one the in-scope CNN encoder uses)."""

    def __init__(self, cnn_method: str, in_channels: int, cnn_kernel_num: int, cnn_window_size: int):
        super().__init__()
        assert cnn_method == 'naive', 'only cnn_method=naive is on the hot path (SURVEY.md section 2, row 5)'
        self.cnn_method = cnn_method
        self.conv = nn.Conv1d(in_channels=in_channels, out_channels=cnn_kernel_num, kernel_size=cnn_window_size,
                              padding=(cnn_window_size - 1) // 2)


class Conv2D_Pool(nn.Module):
    """layers.py:47-79, 'naive' branch (parameter holder: functional.KcnnFn evaluates relu(conv) and the max over the first
    length - cnn_window_size + 1 positions)."""

    def __init__(self, cnn_method: str, in_channels: int, cnn_kernel_num: int, cnn_window_size: int, last_channel_num: int):
        super().__init__()
        assert cnn_method == 'naive', 'only cnn_method=naive is on the hot path (SURVEY.md section 2, row 5)'
        self.cnn_method = cnn_method
        self.in_channels = in_channels
        self.last_channel_num = last_channel_num
        self.cnn_window_size = cnn_window_size
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=cnn_kernel_num, kernel_size=[cnn_window_size, last_channel_num],
                              padding=[(cnn_window_size - 1) // 2, 0])


class GCNLayer(nn.Module):
    """layers.py:265-292 (parameter holder; SUE's pipeline evaluates relu(A (X W^T) + b) + X)."""

    def __init__(self, in_dim, out_dim, residual=False, layer_norm=False):
        super().__init__()
        if residual and in_dim != out_dim:
            raise Exception('To facilitate residual connection, in_dim must equal to out_dim')
        self.residual = residual
        self.layer_norm = layer_norm
        self.W = nn.Linear(in_dim, out_dim, bias=True)
        if self.layer_norm:
            self.layer_normalization = nn.LayerNorm(normalized_shape=[out_dim])       # layers.py:273-274

    def initialize(self):
        nn.init.xavier_uniform_(self.W.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.W.bias)


class GCN(nn.Module):
    """layers.py:294-323."""

    def __init__(self, in_dim, out_dim, hidden_dim=0, num_layers=1, dropout=0.1, residual=False, layer_norm=False):
        super().__init__()
        assert in_dim == out_dim and (num_layers == 1 or hidden_dim == in_dim)
        self.num_layers = num_layers
        self.dropout_rate = float(dropout)
        self.residual = residual
        self.gcn_layers = nn.ModuleList([GCNLayer(in_dim, in_dim, residual=residual, layer_norm=layer_norm) for _ in range(num_layers)])

    def initialize(self):
        for gcn_layer in self.gcn_layers:
            gcn_layer.initialize()

    def forward(self, feature, graph):
        """layers.py:318-323 on its own (the SUE pipeline drives the same kernels directly): feature [B, G, D], graph [B, G, G]."""
        from .user_encoders import _GCNFunction
        return _GCNFunction.apply(feature, self, graph)
