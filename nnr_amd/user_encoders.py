"""User encoders of the hot path (reference: userEncoders.py) on the HIP kernels.

SUE (userEncoders.py:42-98):
  X0 = [history news reps ; dropout_(proxy nodes)]                                   (sue_x0 kernel)
  L x { X <- dropout(relu(A (X W^T) + b) + X) }   -- the dense GEMM first, then the per-user 68x68 aggregate as a batched
                                                     GEMM whose epilogue applies bias / relu / residual / dropout
  gfeat = (GCN(X0) + X0)[:, :50]
  intra-cluster attention: torch_scatter's scatter_softmax / scatter_sum -> sue_intra kernel (segmented LDS reduction;
  the key projection is evaluated once per history item, not on the N-times expanded tensor -- identical math)
  F <- dropout(relu(F W_c^T + b_c) + F)  (GEMM epilogue) ; inter-cluster ScaledDotProduct attention in GEMV form + pool.
Backward is hand-written against the same kernels; parameter gradients accumulate into `param.grad`."""
import math

import torch
import torch.nn as nn

from . import ops
from .layers import Attention, CandidateAttention, ScaledDotProduct_CandidateAttention, MultiHeadAttention, GCN, GRUParams, grad_of, _CandAttnFn
from .news_encoders import NewsEncoder


class UserEncoder(nn.Module):
    """userEncoders.py:12-39: holds a reference to the SAME news-encoder instance (:16)."""
    needs_user_embedding = False         # True: encode_user takes the user embedding rows as a seventh argument (model.Model passes them)
    candidate_independent = False        # True: encode_user expands ONE vector per user over the candidates and never reads them (listwise evaluation
                                         # then encodes a user once per impression, evaluate.compute_scores_listwise)
    needs_history_graph = False          # True: encode_user reads the graph / cluster inputs (evaluate._encoded_users builds them per batch)
    pool_archives = False                # True: the click score of a (user, news) pair is a softmax-weighted sum over the inner products of the
                                         # news with A candidate-free vectors per user (encode_archives, archive_scale): with archives=True evaluate.recommend
                                         # and rank_in_pool rank a whole pool for such an encoder although it is not candidate_independent

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__()
        self.news_embedding_dim = news_encoder.news_embedding_dim
        self.news_encoder = news_encoder
        self.auxiliary_loss = None
        self._seed_base = int(getattr(config, 'seed', 0)) * 104723 + 29
        self._calls = 0

    def _next_seed(self):
        self._calls += 1
        return (self._seed_base + 15485863 * self._calls) & 0x7FFFFFFF

    def forward(self, user_title_text, user_title_mask, user_title_entity, user_content_text, user_content_mask, user_content_entity,
                user_category, user_subCategory, user_history_mask, user_history_graph, user_history_category_mask,
                user_history_category_indices, user_embedding, candidate_news_representation):
        history_embedding = self.news_encoder(user_title_text, user_title_mask, user_title_entity, user_content_text, user_content_mask,
                                              user_content_entity, user_category, user_subCategory, user_embedding)
        extra = (user_embedding,) if self.needs_user_embedding else ()
        return self.encode_user(history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                                user_history_category_indices, candidate_news_representation, *extra)


class _SUEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hist, cand, mod, graph, cmask, cidx):
        out, saved = sue_forward(mod, hist.contiguous(), cand.contiguous(), graph, cmask, cidx)
        ctx.mod, ctx.saved = mod, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        dhist, dcand = sue_backward(ctx.mod, ctx.saved, dout.contiguous())
        ctx.saved = None
        return dhist, dcand, None, None, None, None


# round 4: the candidate-side projections (inputs: the candidates only) and the candidate gradient's accumulations (read by nobody before the news
# encoder's backward) leave SUE's dependent chain for a side stream
_SIDE = {}
ops.STREAM_CACHES.append(_SIDE)


def _sue_side(dev):
    if ops.ONE_STREAM[0]:
        return None
    key = (dev.type, dev.index)
    if key not in _SIDE:
        _SIDE[key] = ops.new_stream(dev)
    return _SIDE[key]


def gcn_forward(gcn, x0, graph, seed0, training):
    """GCN.forward (layers.py:318-323) over GCNLayer.forward (:285-292):  X <- dropout(relu(LN?((A X) W^T + b)) + X).  The dense
    product runs first (X W^T on all B*G rows), then the per-user G x G aggregate as a batched GEMM whose epilogue applies bias /
    relu / residual / dropout -- or, with --gcn_layer_norm, only the bias, followed by the fused LayerNorm kernel."""
    B, G, D = x0.shape
    f32 = dict(device=x0.device, dtype=torch.float32)
    Lg = gcn.num_layers
    xs, rs, lns = [x0], [], []
    x = x0
    for l, layer in enumerate(gcn.gcn_layers):
        y = torch.empty((B, G, D), **f32)
        r = torch.empty((B, G, D), **f32)
        pl = (gcn.dropout_rate if training else 0.0) if l + 1 < Lg else 0.0
        z = ops.linear_fwd(x.view(B * G, D), layer.W.weight)                       # X W^T  (bias goes after the aggregate)
        if getattr(layer, 'layer_norm', False):
            u = torch.empty((B, G, D), **f32)
            ops.gemm(graph, z, u, M=G, N=D, K=G, lda=G, ldb=D, ldc=D, trans_b=True, bias=layer.W.bias, batch=B, strideA=G * G, strideB=G * D,
                     strideC=G * D, tile=2)
            xhat = torch.empty((B, G, D), **f32)
            rstd = torch.empty(B * G, **f32)
            ln = layer.layer_normalization
            ops.layernorm_fwd(u, ln.weight, ln.bias, ln.eps, xhat, rstd, r, x if gcn.residual else None, y, pl, seed0 + l)
            lns.append((xhat, rstd))
        elif G <= 128 and D % 4 == 0:                                              # dedicated per-user aggregate kernel
            ops.gcn_aggregate_fwd(graph, z, layer.W.bias, x if gcn.residual else None, r, y, B, G, D, True, pl, seed0 + l)
            lns.append(None)
        else:
            ops.gemm(graph, z, y, M=G, N=D, K=G, lda=G, ldb=D, ldc=D, trans_b=True, bias=layer.W.bias, act=ops.ACT_RELU, aux_out=r,
                     ldaux=D, resid=x if gcn.residual else None, ldres=D, drop=(3, pl, seed0 + l, D), batch=B, strideA=G * G,
                     strideB=G * D, strideC=G * D, stride_aux=G * D, stride_res=G * D, tile=2)
            lns.append(None)
        xs.append(y)
        rs.append(r)
        x = y
    return x, dict(xs=xs, rs=rs, lns=lns, seed0=seed0, training=training)


def gcn_backward(gcn, gsv, dy, graph, leaf):
    """Gradient of gcn_forward wrt its input; parameter gradients are accumulated (the weight-gradient GEMMs through `leaf`)."""
    B, G, D = dy.shape
    f32 = dict(device=dy.device, dtype=torch.float32)
    Lg = gcn.num_layers
    for l in range(Lg - 1, -1, -1):
        layer = gcn.gcn_layers[l]
        pl = (gcn.dropout_rate if gsv['training'] else 0.0) if l + 1 < Lg else 0.0
        dS = torch.empty((B, G, D), **f32)
        dx = torch.empty((B, G, D), **f32)
        if G <= 128 and D % 4 == 0 and gsv['lns'][l] is None:
            # mask + ReLU gradient applied while dY is loaded, then dZ_b = A_b^T dS_b, one launch (csrc/gcn.hip)
            dz = torch.empty((B, G, D), **f32)
            ops.gcn_aggregate_bwd(graph, dy, gsv['rs'][l], dS, dx if gcn.residual else None, dz, B, G, D, pl, gsv['seed0'] + l)
            ops.linear_bwd_data(dz.view(B * G, D), layer.W.weight, out=dx.view(B * G, D), accumulate=bool(gcn.residual))
            leaf(lambda dS=dS, dz=dz, l=l, layer=layer: (ops.bias_grad(dS.view(B * G, D), grad_of(layer.W.bias)),
                                                         ops.linear_bwd_weight(dz.view(B * G, D), gsv['xs'][l].view(B * G, D), grad_of(layer.W.weight))), dS, dz)
            dy = dx
            continue
        ops.relu_drop_bwd(dy, gsv['rs'][l], dS, dx, pl, gsv['seed0'] + l)        # dx = masked dy (residual branch)
        if not gcn.residual:
            ops.fill_zero(dx)            # (a C-ABI call, not dx.zero_(): a torch fill is not part of a recorded launch tape -- round-3 advisor)
        if gsv['lns'][l] is not None:                                              # through the LayerNorm: dS := d(A z + b)
            xhat, rstd = gsv['lns'][l]
            ln = layer.layer_normalization
            du = torch.empty((B, G, D), **f32)
            ops.layernorm_bwd(dS, xhat, rstd, ln.weight, du, grad_of(ln.weight), grad_of(ln.bias))
            dS = du
        dz = torch.empty((B, G, D), **f32)                                   # dZ_b = A_b^T dS_b
        ops.gemm(graph, dS, dz, M=G, N=D, K=G, lda=G, ldb=D, ldc=D, trans_a=True, trans_b=True, batch=B, strideA=G * G, strideB=G * D,
                 strideC=G * D, tile=2)
        ops.linear_bwd_data(dz.view(B * G, D), layer.W.weight, out=dx.view(B * G, D), accumulate=True)
        leaf(lambda dS=dS, dz=dz, l=l, layer=layer: (ops.bias_grad(dS.view(B * G, D), grad_of(layer.W.bias)),
                                                     ops.linear_bwd_weight(dz.view(B * G, D), gsv['xs'][l].view(B * G, D), grad_of(layer.W.weight))), dS, dz)
        dy = dx
    return dy


class _GCNFunction(torch.autograd.Function):
    """GCN.forward as a standalone layer (layers.GCN.forward)."""

    @staticmethod
    def forward(ctx, feature, gcn, graph):
        seed = (getattr(gcn, '_calls', 0) * 7919 + 101) & 0x7FFFFFFF
        gcn.__dict__['_calls'] = getattr(gcn, '_calls', 0) + 1
        out, gsv = gcn_forward(gcn, feature.contiguous(), graph.contiguous(), seed, gcn.training)
        ctx.gcn, ctx.gsv, ctx.graph = gcn, gsv, graph.contiguous()
        return out

    @staticmethod
    def backward(ctx, dy):
        with ops.leaf_scope(dy.device, enable=False) as leaf:
            dx = gcn_backward(ctx.gcn, ctx.gsv, dy.contiguous(), ctx.graph, leaf)
        ctx.gsv = None
        return dx, None, None


CAPTURE = [None]      # diagnostics / parity tests: set CAPTURE[0] = [] and every sue_forward appends its saved state (ReLU outputs of the GCN
                      # layers in sv['gcn']['rs'], of the cluster affine in sv['rc']); a replayed step rewrites the SAME buffers


# ---------------------------------------------------------------------------------------------------------------------------------------
# SUE's pipeline in stages, each a forward / backward pair written once:  GCN feature -> intra-cluster attention (two forms) -> tail (cluster
# affine + inter-cluster pool).  SUE runs all three, SUE_wo_GCN the last two on the raw history rows, SUE_wo_HCA the first alone.

def _fix_cluster_mask(cmask, fused=None):
    """user_history_category_mask[:, -1] = 1, in place on the caller's tensor (userEncoders.py:73, variantEncoders.py:369).  fused: the
    (B, Kc + 1) shape at which ops.sue_x0_fwd writes the column in its own launch: the mask is then returned for that launch's cmask_fix and
    nothing is issued here.  Otherwise the column is written now (a C-ABI call where the layout allows: recordable) and None is returned."""
    flat = cmask.is_cuda and cmask.dim() == 2 and cmask.is_contiguous()
    if flat and fused is not None and tuple(cmask.shape) == fused:
        return cmask
    if flat and cmask.element_size() == 1:
        ops.fill_column_u8(cmask, -1, 1)
    else:
        cmask[:, -1] = 1
    return None


def gcn_feature_fwd(mod, hist, graph, p, seed, cmask_fix=None):
    """(gcn([history ; dropout_(proxy nodes)]) + X0)[:, :Hn] (userEncoders.py:80-82, variantEncoders.py:414-416).  Dropout sites: the proxy
    nodes at seed + 1, GCN layer l at seed + 10 + l with p / 2.  -> gfeat [B, Hn, D], the GCN's saved state."""
    B, Hn, D = hist.shape
    Kc = mod.proxy_node_embedding.shape[0]
    G = Hn + Kc
    f32 = dict(device=hist.device, dtype=torch.float32)
    x0 = torch.empty((B, G, D), **f32)
    ops.sue_x0_fwd(hist, mod.proxy_node_embedding, x0, B, Hn, Kc, D, p, seed + 1, cmask_fix=cmask_fix)
    x, gsv = gcn_forward(mod.gcn, x0, graph, seed + 10, mod.training)
    gfeat = torch.empty((B, Hn, D), **f32)
    ops.sue_slice_fwd(x, x0, gfeat, B, Hn, G, D)
    return gfeat, gsv


def gcn_feature_bwd(mod, gsv, graph, dg, p, seed, leaf, dhist_out=None):
    """dg [B, Hn, D] -> the history gradient (written to dhist_out if given); GCN and proxy-node gradients accumulate into .grad."""
    B, Hn, D = dg.shape
    Kc = mod.proxy_node_embedding.shape[0]
    G = Hn + Kc
    f32 = dict(device=dg.device, dtype=torch.float32)
    dpad = torch.empty((B, G, D), **f32)
    ops.sue_slice_bwd(dg, dpad, B, Hn, G, D)
    dy = gcn_backward(mod.gcn, gsv, dpad, graph, leaf)
    dhist = torch.empty((B, Hn, D), **f32) if dhist_out is None else dhist_out
    ops.sue_x0_bwd(dy, dhist, grad_of(mod.proxy_node_embedding), B, Hn, Kc, D, p, seed + 1, dx0_add=dpad)      # d(gcn(X0) + X0)
    return dhist


class _IntraKeys:
    """Intra-cluster attention on a projected key buffer (ops.sue_intra_*): the key projection is evaluated once per history item."""
    cand_widths = staticmethod(lambda A, D: dict(qc=A))

    @staticmethod
    def cand_fwd(mod, cand2, cs):
        ops.linear_fwd(cand2, mod.intraCluster_Q.weight, mod.intraCluster_Q.bias, out=cs['qc'])         # [B*N, A]

    @staticmethod
    def fwd(mod, x, cand_ready, cidx, N, Cn):
        B, Hn, D = x.shape
        A = mod.attention_dim
        f32 = dict(device=x.device, dtype=torch.float32)
        kf = ops.linear_fwd(x.view(B * Hn, D), mod.intraCluster_K.weight)                               # [B*Hn, A]
        cs = cand_ready()
        alpha_i = torch.empty((B, N, Hn), **f32)
        feat = torch.empty((B * N * Cn, D), **f32)
        ops.sue_intra_fwd(kf, cs['qc'], x, cidx, B, N, Hn, Cn, A, D, alpha_i, feat)
        return alpha_i, feat, dict(kf=kf)

    @staticmethod
    def bwd(mod, sv, dfeat, dcand, leaf, on_side):
        B, Hn, D, N, Cn, A = (sv[k] for k in ('B', 'Hn', 'D', 'N', 'Cn', 'A'))
        f32 = dict(device=dfeat.device, dtype=torch.float32)
        cand2 = sv['cand'].view(B * N, D)
        dg = torch.empty((B, Hn, D), **f32)
        dkf = torch.empty((B * Hn, A), **f32)
        dqc = torch.empty((B * N, A), **f32)
        ops.sue_intra_bwd(sv['kf'], sv['qc'], sv['x'], sv['cidx'], sv['alpha_i'], dfeat, B, N, Hn, Cn, A, D, dg, dkf, dqc)
        ops.linear_bwd_data(dkf, mod.intraCluster_K.weight, out=dg.view(B * Hn, D), accumulate=True)
        on_side(lambda: ops.linear_bwd_data(dqc, mod.intraCluster_Q.weight, out=dcand, accumulate=True))
        leaf(lambda: (ops.linear_bwd_weight(dkf, sv['x'].view(B * Hn, D), grad_of(mod.intraCluster_K.weight)),
                      ops.linear_bwd_weight(dqc, cand2, grad_of(mod.intraCluster_Q.weight), db=grad_of(mod.intraCluster_Q.bias))), dkf, dqc)
        return dg


class _IntraGemv:
    """Intra-cluster attention in GEMV form (ops.sue_seg_pool_*): a bias of intraCluster_K shifts every score of a (user, candidate) alike and
    cancels in each segment softmax, so the scores are x_h . u_n / sqrt(A) with u = Q(c) W_K -- one [B N, A] x [A, D] product instead of the
    [B Hn, D] x [D, A] key projection and its two backward products.  The bias' gradient is exactly zero."""
    cand_widths = staticmethod(lambda A, D: dict(qc=A, u=D))

    @staticmethod
    def cand_fwd(mod, cand2, cs):
        A, D = cs['qc'].shape[1], cs['u'].shape[1]
        ops.linear_fwd(cand2, mod.intraCluster_Q.weight, mod.intraCluster_Q.bias, out=cs['qc'])         # [B*N, A]
        ops.gemm(cs['qc'], mod.intraCluster_K.weight, cs['u'], M=cand2.shape[0], N=D, K=A, lda=A, ldb=D, ldc=D, trans_b=True)   # W_K^T q

    @staticmethod
    def fwd(mod, x, cand_ready, cidx, N, Cn):
        B, Hn, D = x.shape
        f32 = dict(device=x.device, dtype=torch.float32)
        cs = cand_ready()
        alpha_i = torch.empty((B, N, Hn), **f32)
        feat = torch.empty((B * N * Cn, D), **f32)
        ops.sue_seg_pool_fwd(x, cs['u'], cidx, B, N, Hn, Cn, D, 1.0 / math.sqrt(mod.attention_dim), alpha_i, feat)
        return alpha_i, feat, {}

    @staticmethod
    def bwd(mod, sv, dfeat, dcand, leaf, on_side):
        B, Hn, D, N, Cn, A = (sv[k] for k in ('B', 'Hn', 'D', 'N', 'Cn', 'A'))
        f32 = dict(device=dfeat.device, dtype=torch.float32)
        cand2 = sv['cand'].view(B * N, D)
        dx = torch.empty((B, Hn, D), **f32)
        du = torch.empty((B * N, D), **f32)
        ops.sue_seg_pool_bwd(sv['x'], sv['u'], sv['cidx'], sv['alpha_i'], dfeat, B, N, Hn, Cn, D, 1.0 / math.sqrt(A), dx, du)
        dqc = torch.empty((B * N, A), **f32)
        ops.gemm(du, mod.intraCluster_K.weight, dqc, M=B * N, N=A, K=D, lda=D, ldb=D, ldc=A)           # du W_K^T
        if mod.intraCluster_K.bias is not None:
            grad_of(mod.intraCluster_K.bias)                                                            # (exactly zero: the bias cancels)
        leaf(lambda: (ops.linear_bwd_weight(sv['qc'], du, grad_of(mod.intraCluster_K.weight)),
                      ops.linear_bwd_weight(dqc, cand2, grad_of(mod.intraCluster_Q.weight), db=grad_of(mod.intraCluster_Q.bias))), du, dqc)
        on_side(lambda: ops.linear_bwd_data(dqc, mod.intraCluster_Q.weight, out=dcand, accumulate=True))
        return dx


def _tail_cand_fwd(mod, cand2, cs):
    """q and v of the inter-cluster attention (layers.py:196-203 in GEMV form): inputs are the candidates only."""
    ia = mod.interClusterAttention
    A, D = cs['qv'].shape[1], cs['v'].shape[1]
    ops.linear_fwd(cand2, ia.Q.weight, ia.Q.bias, out=cs['qv'])                                          # [B*N, A]
    ops.gemm(cs['qv'], ia.K.weight, cs['v'], M=cand2.shape[0], N=D, K=A, lda=A, ldb=D, ldc=D, trans_b=True)


def _tail_fwd(mod, feat, v, cmask, N, p, seed):
    """F <- dropout(relu(F W_c^T + b_c) + F) (GEMM epilogue, dropout site seed + 2, flat over [B N C, D]), then the inter-cluster pool."""
    R, D = feat.shape
    Cn = R // v.shape[0]
    f32 = dict(device=feat.device, dtype=torch.float32)
    aff = mod.clusterFeatureAffine
    rc = torch.empty((R, D), **f32)
    f2 = torch.empty((R, D), **f32)
    ops.gemm(feat, aff.weight, f2, M=R, N=D, K=D, lda=D, ldb=D, ldc=D, bias=aff.bias, act=ops.ACT_RELU, aux_out=rc, ldaux=D, resid=feat, ldres=D,
             drop=(3, p, seed + 2, D))
    alpha_o = torch.empty(R, **f32)
    out = torch.empty((v.shape[0], D), **f32)
    ops.pool_fwd(x=f2, ldx=D, D=D, n=v.shape[0], Lx=Cn, mask=cmask, mask_div=N, v=v, ldv=D, scale=1.0 / math.sqrt(mod.attention_dim), alpha=alpha_o,
                 out=out, ldo=D)
    return out, dict(rc=rc, f2=f2, alpha_o=alpha_o)


def _tail_bwd(mod, sv, dout, leaf, on_side, dcand_accum=None):
    """dout [B*N, D] -> (d cluster features [B*N*Cn, D], the candidate gradient so far).  dcand_accum [B*N, D] (optional): the candidate gradient
    is ADDED into it.  Nobody reads the candidate gradient (or d q_v) before the news encoder's backward: those launches go through on_side."""
    B, D, N, Cn, A, p, seed = (sv[k] for k in ('B', 'D', 'N', 'Cn', 'A', 'p', 'seed'))
    f32 = dict(device=dout.device, dtype=torch.float32)
    cand2 = sv['cand'].view(B * N, D)
    ia, aff = mod.interClusterAttention, mod.clusterFeatureAffine
    # ---- inter-cluster pool
    df2 = torch.empty((B * N * Cn, D), **f32)
    dv = torch.empty((B * N, D), **f32)
    ops.pool_bwd(x=sv['f2'], ldx=D, D=D, n=B * N, Lx=Cn, mask=sv['cmask'], mask_div=N, v=sv['v'], ldv=D, scale=1.0 / math.sqrt(A),
                 alpha=sv['alpha_o'], dout=dout, lddo=D, dx=df2, lddx=D, dv=dv, lddv=D)
    dqv = torch.empty((B * N, A), **f32)
    # the step without autograd: the candidate gradient goes straight into the union gradient buffer's candidate rows
    dcand = dcand_accum if dcand_accum is not None else torch.empty((B * N, D), **f32)

    def inter_q():
        ops.gemm(dv, ia.K.weight, dqv, M=B * N, N=A, K=D, lda=D, ldb=D, ldc=A)
        leaf(lambda: (ops.linear_bwd_weight(sv['qv'], dv, grad_of(ia.K.weight)),
                      ops.linear_bwd_weight(dqv, cand2, grad_of(ia.Q.weight), db=grad_of(ia.Q.bias))), dv, dqv)
        ops.linear_bwd_data(dqv, ia.Q.weight, out=dcand, accumulate=dcand_accum is not None)             # [B*N, D]
    on_side(inter_q)
    # ---- cluster affine
    dS = torch.empty((B * N * Cn, D), **f32)
    dfeat = torch.empty((B * N * Cn, D), **f32)
    ops.relu_drop_bwd(df2, sv['rc'], dS, dfeat, p, seed + 2)
    ops.linear_bwd_data(dS, aff.weight, out=dfeat, accumulate=True)
    # (Measured and rejected in round 3: handing the five 900 x 900 weight-gradient GEMMs of this encoder to the news encoder's backward,
    # to run beside the backward recurrence on the 19 KB tile instead of beside this chain's data-gradient GEMMs: 11.41-11.43 vs
    # 11.19-11.25 ms/step.)
    leaf(lambda: ops.linear_bwd_weight(dS, sv['feat'], grad_of(aff.weight), db=grad_of(aff.bias)), dS)
    return dfeat, dcand


def _cluster_fwd(mod, hist, cand, cmask, cidx, side, features):
    """Intra stage (mod.intra_form) + tail on the rows features(sv) returns (called after the candidate-side launches have been issued on `side`;
    it also fixes the cluster mask).  side: a stream for the candidate-side projections -- three or four small launches (15-30 us each,
    latency-bound) that need nothing but `cand` and would sit on the dependent chain -- or None: they are issued where the first is read."""
    form = mod.intra_form
    B, Hn, D = hist.shape
    N, Cn, A = cand.shape[1], mod.category_num, mod.attention_dim
    dev = hist.device
    f32 = dict(device=dev, dtype=torch.float32)
    p = mod.dropout_rate if mod.training else 0.0
    seed = mod._next_seed()
    sv = dict(B=B, Hn=Hn, D=D, N=N, Cn=Cn, A=A, p=p, seed=seed, hist=hist, cand=cand, cidx=cidx, cmask=cmask)
    cand2 = cand.view(B * N, D)
    cs = {k: torch.empty((B * N, w), **f32) for k, w in dict(form.cand_widths(A, D), qv=A, v=D).items()}

    def cand_side():
        form.cand_fwd(mod, cand2, cs)
        _tail_cand_fwd(mod, cand2, cs)
    side_ev = None
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            cand_side()
            side_ev = torch.cuda.Event()
            side_ev.record()

    def cand_ready():
        if side is None:
            cand_side()
        else:
            torch.cuda.current_stream(dev).wait_event(side_ev)
        return cs
    x = features(sv)
    alpha_i, feat, isv = form.fwd(mod, x, cand_ready, cidx, N, Cn)
    out, tsv = _tail_fwd(mod, feat, cs['v'], cmask, N, p, seed)
    sv.update(cs, x=x, alpha_i=alpha_i, feat=feat, **isv, **tsv)
    return out.view(B, N, D), sv


def _cluster_bwd(mod, sv, dout, leaf, side, dcand_accum=None):
    """-> (gradient of the intra stage's history rows, candidate gradient [B*N, D]).  With a side stream the candidate gradient is complete once
    the caller has made its stream wait for `side`."""
    B, N, D = sv['B'], sv['N'], sv['D']
    main = torch.cuda.current_stream(dout.device)

    def on_side(fn):
        if side is None:
            return fn()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            return fn()
    dfeat, dcand = _tail_bwd(mod, sv, dout.view(B * N, D), leaf, on_side, dcand_accum)
    return mod.intra_form.bwd(mod, sv, dfeat, dcand, leaf, on_side), dcand


def sue_forward(mod, hist, cand, graph, cmask, cidx):
    def features(sv):
        # (the in-place `user_history_category_mask[:, -1] = 1` of userEncoders.py:73 in sue_x0_fwd's launch where the mask's layout allows)
        Kc = mod.proxy_node_embedding.shape[0]
        fix = _fix_cluster_mask(cmask, (sv['B'], Kc + 1))
        gfeat, gsv = gcn_feature_fwd(mod, hist, graph, sv['p'], sv['seed'], cmask_fix=fix)
        sv.update(Kc=Kc, G=sv['Hn'] + Kc, graph=graph, gcn=gsv, gfeat=gfeat)
        return gfeat
    out, sv = _cluster_fwd(mod, hist, cand, cmask, cidx, _sue_side(hist.device), features)
    if CAPTURE[0] is not None:
        CAPTURE[0].append(sv)
    return out, sv


def sue_backward(mod, sv, dout, dhist_out=None, dcand_accum=None):
    """dhist_out [B, Hn, D] (optional): where the history gradient is written; dcand_accum [B*N, D] (optional): the candidate
    gradient is ADDED into it (the step without autograd sums the click predictor's and this encoder's share there)."""
    dev = dout.device
    hook = mod.__dict__.get('_grads_ready_hook')
    # a data-parallel trainer starts reducing this encoder's gradients right after this function (early bucket): then they must be
    # ordered on the current stream when it returns.  Otherwise nobody needs them before the optimizer: the leaf stream is joined at
    # the end of the backward pass, and the news encoder's backward starts without waiting for the last weight-gradient GEMMs (round 4, joined
    # vs deferred: batch 8 3.33-3.40 vs 3.20-3.21 ms -- the main stream sat idle for ~200 us behind four 65 us GEMMs --, batch 64 10.47-10.55 vs 10.43-10.49)
    exchange = getattr(hook, '__self__', None)
    need_now = (exchange is not None and exchange.active()) or not ops._DEFER.get('step_joins')      # (only the native step ends with its own join)
    side = _sue_side(dev)
    with ops.leaf_scope(dev, defer_join=not need_now) as leaf:
        dg, dcand = _cluster_bwd(mod, sv, dout, leaf, side, dcand_accum)
        dhist = gcn_feature_bwd(mod, sv['gcn'], sv['graph'], dg, sv['p'], sv['seed'], leaf, dhist_out)
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)      # the candidate gradient is complete
    # (joined form) every parameter gradient of this encoder is now ordered on the current stream:
    # a data-parallel trainer starts reducing them while the news encoder's backward is still to come (dp.GradientExchange).
    # (Measured and rejected: issuing this encoder's weight-gradient GEMMs only after its data-gradient chain, so that they
    # overlap the news encoder's backward prologue instead of slowing the 4 352-row chain: 13.05 vs 12.84 ms/step.)
    if hook is not None:
        hook()
    return dhist, dcand.view(sv['B'], sv['N'], sv['D'])


def _cluster_layers(mod, config, key_bias):
    """The layers of the hierarchical cluster attention (userEncoders.py:52-60, variantEncoders.py:349-358), registered in the reference's order."""
    D = mod.news_embedding_dim
    mod.attention_dim = max(config.attention_dim, D // 4)
    mod.intraCluster_K = nn.Linear(D, mod.attention_dim, bias=key_bias)
    mod.intraCluster_Q = nn.Linear(D, mod.attention_dim, bias=True)
    mod.clusterFeatureAffine = nn.Linear(D, D, bias=True)
    mod.interClusterAttention = ScaledDotProduct_CandidateAttention(D, D, mod.attention_dim)
    mod.dropout_rate = float(config.dropout_rate)
    mod.category_num = config.category_num + 1     # extra one category index for padding news
    mod.max_history_num = config.max_history_num
    mod.attention_scalar = math.sqrt(float(mod.attention_dim))


def _cluster_layers_initialize(mod):
    nn.init.xavier_uniform_(mod.intraCluster_K.weight)
    if mod.intraCluster_K.bias is not None:
        nn.init.zeros_(mod.intraCluster_K.bias)
    nn.init.xavier_uniform_(mod.intraCluster_Q.weight)
    nn.init.zeros_(mod.intraCluster_Q.bias)
    nn.init.xavier_uniform_(mod.clusterFeatureAffine.weight, gain=nn.init.calculate_gain('relu'))
    nn.init.zeros_(mod.clusterFeatureAffine.bias)
    mod.interClusterAttention.initialize()


class SUE(UserEncoder):
    """userEncoders.py:42-98."""
    needs_history_graph = True           # evaluate._encoded_users builds the graph / cluster inputs for such an encoder
    intra_form = _IntraKeys              # what the cluster pipeline runs as its intra stage (as _CNEAblation states what it keeps)

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.proxy_node_embedding = nn.Parameter(torch.zeros([config.category_num, self.news_embedding_dim]))
        self.gcn = GCN(in_dim=self.news_embedding_dim, out_dim=self.news_embedding_dim, hidden_dim=self.news_embedding_dim,
                       num_layers=config.gcn_layer_num, dropout=config.dropout_rate / 2, residual=not config.no_gcn_residual,
                       layer_norm=config.gcn_layer_norm)
        _cluster_layers(self, config, key_bias=False)

    def initialize(self):
        self.gcn.initialize()
        nn.init.zeros_(self.proxy_node_embedding)
        _cluster_layers_initialize(self)

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        """Everything of forward() after the history news have been encoded (userEncoders.py:73-75, 79-98)."""
        # (user_history_category_mask[:, -1] = 1, in place on the caller's tensor, userEncoders.py:73: done by sue_forward's first launch)
        graph = user_history_graph.contiguous()
        cidx = user_history_category_indices.contiguous()
        assert cidx.dtype == torch.int64 and graph.dtype == torch.float32
        return _SUEFunction.apply(history_embedding, candidate_news_representation, self, graph, user_history_category_mask, cidx)


class _SueWoGcnFn(torch.autograd.Function):
    """SUE_wo_GCN after the news encoder (variantEncoders.py:369-390): SUE's pipeline from the intra-cluster attention on, straight on the
    history representations, on one stream.  Parameter gradients accumulate into .grad (weight-gradient GEMMs on the leaf stream, joined
    before this returns); the data-parallel early-bucket hook is SUE's alone and is not fired here."""

    @staticmethod
    def forward(ctx, hist, cand, mod, cmask, cidx):
        def features(sv):
            _fix_cluster_mask(cmask)
            return sv['hist']
        out, ctx.saved = _cluster_fwd(mod, hist.contiguous(), cand.contiguous(), cmask, cidx, None, features)
        ctx.mod = mod
        return out

    @staticmethod
    def backward(ctx, dout):
        mod, sv = ctx.mod, ctx.saved
        ctx.saved = None
        with ops.leaf_scope(dout.device) as leaf:
            dhist, dcand = _cluster_bwd(mod, sv, dout.contiguous(), leaf, None)
        return dhist, dcand.view(sv['B'], sv['N'], sv['D']), None, None, None


class SUE_wo_GCN(UserEncoder):
    """variantEncoders.py:342-390, the ablation of SUE without the GCN: hierarchical cluster attention on the news encoder's history output
    (no proxy nodes, no graph, no slice).  intraCluster_K carries the reference's bias, which cannot change the output (see _IntraGemv): it
    stays a parameter so that a reference state_dict loads unchanged, and its gradient is exactly zero."""
    needs_history_graph = True
    intra_form = _IntraGemv

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        _cluster_layers(self, config, key_bias=True)
        if not ops.seg_pool_supported(self.max_history_num, self.category_num, config.negative_sample_num + 1):
            raise Exception('SUE_wo_GCN: ' + ops.SEG_POOL_UNSUPPORTED)

    def initialize(self):
        _cluster_layers_initialize(self)

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        cidx = user_history_category_indices.contiguous()
        assert cidx.dtype == torch.int64
        return _SueWoGcnFn.apply(history_embedding, candidate_news_representation, self, user_history_category_mask, cidx)


class _SueGcnFeatureFn(torch.autograd.Function):
    """The GCN feature stage alone, on SUE's own launches and dropout sites.  The cluster mask is not touched."""

    @staticmethod
    def forward(ctx, hist, mod, graph):
        p = mod.dropout_rate if mod.training else 0.0
        seed = mod._next_seed()
        gfeat, gsv = gcn_feature_fwd(mod, hist.contiguous(), graph, p, seed)
        ctx.mod, ctx.saved = mod, (gsv, graph, p, seed)
        return gfeat

    @staticmethod
    def backward(ctx, dg):
        gsv, graph, p, seed = ctx.saved
        ctx.saved = None
        with ops.leaf_scope(dg.device) as leaf:
            dhist = gcn_feature_bwd(ctx.mod, gsv, graph, dg.contiguous(), p, seed, leaf)
        return dhist, None, None


class SUE_wo_HCA(UserEncoder):
    """variantEncoders.py:393-419, the ablation of SUE without the hierarchical cluster attention: the GCN over [history ; proxy nodes] with
    its outer residual, the first max_history_num rows, one UNMASKED additive attention (padded history slots take part), the user vector
    repeated over the candidates.  Reads neither the candidates nor any mask nor the cluster indices, and does not write the cluster mask."""
    needs_history_graph = True
    candidate_independent = True

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.max_history_num = config.max_history_num
        self.proxy_node_embedding = nn.Parameter(torch.zeros([config.category_num, self.news_embedding_dim]))
        self.gcn = GCN(in_dim=self.news_embedding_dim, out_dim=self.news_embedding_dim, hidden_dim=self.news_embedding_dim,
                       num_layers=config.gcn_layer_num, dropout=config.dropout_rate / 2, residual=not config.no_gcn_residual,
                       layer_norm=config.gcn_layer_norm)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)
        self.dropout_rate = float(config.dropout_rate)

    def initialize(self):
        nn.init.zeros_(self.proxy_node_embedding)
        self.gcn.initialize()
        self.attention.initialize()

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        from . import functional as Fn
        graph = user_history_graph.contiguous()
        assert graph.dtype == torch.float32
        gfeat = _SueGcnFeatureFn.apply(history_embedding, self, graph)
        return Fn.ExpandFn.apply(self.attention(gfeat), candidate_news_representation.size(1))


class MHSA(UserEncoder):
    """userEncoders.py:151-173.  Note F.dropout's default p = 0.5 (not dropout_rate) at :171 and the UNMASKED pool at :172."""
    candidate_independent = True

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.head_num, self.head_dim, self.max_history_num = config.head_num, config.head_dim, config.max_history_num
        self.multiheadAttention = MultiHeadAttention(config.head_num, self.news_embedding_dim, config.max_history_num,
                                                     config.max_history_num, config.head_dim, config.head_dim)
        self.affine = nn.Linear(config.head_num * config.head_dim, self.news_embedding_dim, bias=True)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)

    def initialize(self):
        self.multiheadAttention.initialize()
        nn.init.xavier_uniform_(self.affine.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.affine.bias)
        self.attention.initialize()

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        from . import functional as Fn
        news_num = candidate_news_representation.size(1)
        B, Hn, D = history_embedding.shape
        qkv = Fn.QKVFn.apply(history_embedding.reshape(B * Hn, D), self.multiheadAttention, None)
        h = Fn.MhsaCoreFn.apply(qkv, user_history_mask.contiguous(), B, Hn, self.head_num, self.head_dim)
        # relu(dropout(affine(h))) == dropout(relu(affine(h))): the mask scales by a non-negative factor
        h = Fn.LinearFn.apply(h, self.affine.weight, self.affine.bias, ops.ACT_RELU, 0.5 if self.training else 0.0, self._next_seed())
        user = self.attention(h.view(B, Hn, D))                                                            # unmasked
        return Fn.ExpandFn.apply(user, news_num)

class ATT(UserEncoder):
    """userEncoders.py:176-191: unmasked additive attention over the history slots (padded slots participate)."""
    candidate_independent = True

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)

    def initialize(self):
        self.attention.initialize()

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        from . import functional as Fn
        return Fn.ExpandFn.apply(self.attention(history_embedding), candidate_news_representation.size(1))


class GRU(UserEncoder):
    """userEncoders.py:287-332 (the user encoder of the DAE-GRU baseline): nn.GRU over the first user_history_mask.sum() history slots from
    h = 0, user vector tanh(dec(h_final)), exactly zero for a user without history.  The sort / pack / de-sort of the reference is replaced by
    running every user for t < len and freezing h afterwards (csrc/gru.hip): same values, no planner, no host sync."""
    candidate_independent = True

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        if not ops.gru_supported(config.hidden_dim, config.max_history_num):
            raise Exception('GRU: ' + ops.GRU_UNSUPPORTED)
        self.gru = GRUParams(self.news_embedding_dim, config.hidden_dim)
        self.dec = nn.Linear(config.hidden_dim, self.news_embedding_dim, bias=True)

    def initialize(self):
        """userEncoders.py:293-300: orthogonal_ on each whole [3H, .] matrix, zero GRU biases, xavier_uniform_ (tanh gain) / zeros on dec."""
        for p in self.gru.param_list():
            (nn.init.orthogonal_ if p.dim() >= 2 else nn.init.zeros_)(p.data)
        nn.init.xavier_uniform_(self.dec.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.dec.bias)

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        from . import functional as Fn
        h, length, _ = Fn.GruFn.apply(history_embedding, user_history_mask, self.gru, None)
        user = Fn.GruDecFn.apply(h, self.dec.weight, self.dec.bias, length)
        return Fn.ExpandFn.apply(user, candidate_news_representation.size(1))


class CATT(UserEncoder):
    """userEncoders.py:194-221: candidate-aware additive attention over the click history, one user vector per candidate.
    relu(affine1([cand ; hist])) = relu(Wc cand + b1 + Wh hist) with Wc | Wh the two column halves of affine1.weight (views, no copies: the
    state_dict stays the reference's), so the [B, N, H, 2D] concatenation never exists (layers._CandAttnFn).  A user without history gets the
    reference's uniform weights over all H padded slots.  affine2.bias cancels in the softmax: it exists, and its gradient is exactly zero."""

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.affine1 = nn.Linear(self.news_embedding_dim * 2, config.attention_dim, bias=True)
        self.affine2 = nn.Linear(config.attention_dim, 1, bias=True)
        self.max_history_num = config.max_history_num

    def initialize(self):
        nn.init.xavier_uniform_(self.affine1.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.affine1.bias)
        nn.init.xavier_uniform_(self.affine2.weight)
        nn.init.zeros_(self.affine2.bias)

    def _cand_attn_weights(self):
        D, w = self.news_embedding_dim, self.affine1.weight.detach()
        return w[:, :D], self.affine1.bias, w[:, D:], self.affine2.weight.view(-1), ops.ACT_RELU

    def _cand_attn_grads(self):
        D, g = self.news_embedding_dim, grad_of(self.affine1.weight)
        grad_of(self.affine2.bias)                              # (stays zero)
        return g[:, :D], grad_of(self.affine1.bias), g[:, D:], grad_of(self.affine2.weight).view(-1)

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        return _CandAttnFn.apply(history_embedding, candidate_news_representation, self, user_history_mask)


def _omap_forward(mod, hist, cand, mask):
    """nnr_omap_fwd for hist [B, H, D], cand [B, N, D], mask [B, H] or None: (x, c, mask as passed on, alpha, Y, beta, R, gamma, out, sizes)."""
    B, H, D = hist.shape
    N, K = cand.shape[1], mod.OMAP_head_num
    x = hist if hist.stride(2) == 1 and hist.stride(0) == H * hist.stride(1) else hist.contiguous()
    c = cand.contiguous()
    if mask is not None:
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
    W = mod.W.detach()
    f32 = dict(device=x.device, dtype=torch.float32)
    alpha, Y, beta = torch.empty((B, H, H), **f32), torch.empty((B, H, D), **f32), torch.empty((B, H, K), **f32)
    R, gamma, out = torch.empty((B, K, D), **f32), torch.empty((B, N, K), **f32), torch.empty((B, N, D), **f32)
    ops.omap_fwd(x, c, mask, W, B, N, H, D, K, alpha, Y, beta, R, gamma, out)
    return x, c, mask, alpha, Y, beta, R, gamma, out, (B, N, H, D, K)


class _OmapFn(torch.autograd.Function):
    """hist [B, H, D], cand [B, N, D], mask [B, H] -> [B, N, D] on the kernels of csrc/omap.hip (three launches forward, four backward).  alpha,
    Y = X + alpha X, beta, the archives and gamma are saved; dW goes straight into W.grad."""

    @staticmethod
    def forward(ctx, hist, cand, mod, mask):
        x, c, mask, alpha, Y, beta, R, gamma, out, sizes = _omap_forward(mod, hist, cand, mask)
        ctx.mod, ctx.saved = mod, (x, c, mask, alpha, Y, beta, R, gamma, sizes)
        return out

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        x, c, mask, alpha, Y, beta, R, gamma, (B, N, H, D, K) = ctx.saved
        ctx.saved = None
        f32 = dict(device=x.device, dtype=torch.float32)
        dx, dc = torch.empty((B, H, D), **f32), torch.empty((B, N, D), **f32)
        ops.omap_bwd(x, c, mask, mod.W.detach(), alpha, Y, beta, R, gamma, dout.contiguous(), B, N, H, D, K, dx, dc, grad_of(mod.W))
        return dx, dc, None, None


class _OmapRegFn(torch.autograd.Function):
    """coef * ||(W^T W) o (J - I)||_F as a 0-dim device tensor; its backward adds the gradient into W.grad, scaled by the upstream gradient
    on the device (no host read of the norm in either direction)."""

    @staticmethod
    def forward(ctx, W, mod):
        K = W.shape[1]
        off = torch.empty(K * K + 1, device=W.device, dtype=torch.float32)
        loss = torch.empty((), device=W.device, dtype=torch.float32)
        ops.omap_reg_fwd(W.detach(), mod.HiFi_Ark_regularizer_coefficient, off, loss)
        ctx.mod, ctx.off = mod, off
        return loss

    @staticmethod
    def backward(ctx, g):
        mod = ctx.mod
        ops.omap_reg_bwd(mod.W.detach(), ctx.off, g.contiguous().float(), mod.HiFi_Ark_regularizer_coefficient, grad_of(mod.W))
        return None, None


class OMAP(UserEncoder):
    """userEncoders.py:335-375, the Hi-Fi Ark baseline: self-attention over the history with a residual, K archives pooled by a softmax over
    the heads, one user vector per candidate from a softmax over the archives.  Observable quirks kept: a padded history row has beta = 1/K and
    adds Y[i] / K to every archive; a user without history has alpha = 1/H; masked scores pass no gradient.  In train mode every call
    rewrites `auxiliary_loss` = coefficient * ||(W^T W) o (J_K - I_K)||_F (a 0-dim tensor that carries its own backward); in eval mode it is
    left as it was.  state_dict: W (J_k / I_k are plain attributes, as in the reference).
    pool_archives: the user vector is gamma R with gamma = softmax_k(<R_k, n> / scalar), so the click score <gamma R, n> is
    sum_k gamma_k <R_k, n>: a function of the candidate's inner products with the K archives, which do not depend on it (encode_archives;
    archive_scale = 1 / scalar).  evaluate.recommend / rank_in_pool rank a whole pool on that form when asked to (archives=True)."""
    pool_archives = True

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.max_history_num = config.max_history_num
        self.OMAP_head_num = int(config.OMAP_head_num)
        self.HiFi_Ark_regularizer_coefficient = float(config.HiFi_Ark_regularizer_coefficient)
        self.scalar = math.sqrt(float(self.news_embedding_dim))
        self.archive_scale = 1.0 / self.scalar
        self.W = nn.parameter.Parameter(torch.zeros([self.news_embedding_dim, self.OMAP_head_num]))
        self.J_k = torch.ones([self.OMAP_head_num, self.OMAP_head_num])
        self.I_k = torch.eye(self.OMAP_head_num)

    def initialize(self):
        nn.init.orthogonal_(self.W.data)

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        user_representation = _OmapFn.apply(history_embedding, candidate_news_representation, self, user_history_mask)
        if self.training:
            self.auxiliary_loss = _OmapRegFn.apply(self.W, self)
        return user_representation

    @torch.no_grad()
    def encode_archives(self, history_embedding, user_history_mask):
        """The archives R [B, K, D] that encode_user computes for this history [B, H, D] and mask [B, H], with its bits: the forward entry
        point on one blank candidate per user (R never reads the candidates, and its summation order depends on neither N nor B), the
        quirks included (a padded row adds Y[i] / K to every archive; a user without history has alpha = 1 / H).  No autograd, and
        `auxiliary_loss` stays as it was."""
        B, _, D = history_embedding.shape
        blank = torch.zeros((B, 1, D), device=history_embedding.device, dtype=torch.float32)
        return _omap_forward(self, history_embedding.detach(), blank, user_history_mask)[6]


class PUE(UserEncoder):
    """userEncoders.py:265-284, NPA's personalised user encoder: additive attention over the click history (masked) whose query is
    relu(dense(user_embedding)), the user vector repeated over the candidates.  B problems of max_history_num slots: the shape
    layers.CandidateAttention's kernel (csrc/cand_attn.hip) was built for.  encode_user takes the user embedding rows as a seventh argument
    (needs_user_embedding tells model.Model to pass them)."""
    needs_user_embedding = True
    candidate_independent = True

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        self.dense = nn.Linear(config.user_embedding_dim, config.personalized_embedding_dim, bias=True)
        self.personalizedAttention = CandidateAttention(self.news_embedding_dim, config.personalized_embedding_dim, config.attention_dim)

    def initialize(self):
        nn.init.xavier_uniform_(self.dense.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.dense.bias)
        self.personalizedAttention.initialize()

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation, user_embedding=None):
        from . import functional as Fn
        if user_embedding is None:
            raise Exception('PUE needs the user embedding rows (model.Model passes dropout(user_embedding(user_ID)))')
        q_d = Fn.LinearFn.apply(user_embedding, self.dense.weight, self.dense.bias, ops.ACT_RELU, 0.0, 0)     # [B, personalized_embedding_dim]
        user = self.personalizedAttention(history_embedding, q_d, user_history_mask)                          # [B, news_embedding_dim]
        return Fn.ExpandFn.apply(user, candidate_news_representation.size(1))


class FIM(UserEncoder):
    """userEncoders.py:224-262, fine-grained interest matching: for every candidate, history slot and level of the HDC pair an S x S image
    cand_level^T . hist_level / sqrt(HDC_filter_num) (level 0 too, although it contracts over word_embedding_dim), the four levels as the
    channels of Conv3d over (history, candidate position, history position), elu -> maxpool -> elu -> maxpool -> [B, N, feature_size]
    (functional.FimFn, csrc/fim.hip: each Conv3d + ELU + MaxPool3d is one launch, the dense convolution output never exists).
    `user_history_mask` is not read: padded history slots take part."""

    def __init__(self, news_encoder: NewsEncoder, config):
        super().__init__(news_encoder, config)
        from .news_encoders import HDC
        assert type(self.news_encoder) == HDC, 'For FIM, the news encoder must be HDC'
        self.HDC_sequence_length = news_encoder.HDC_sequence_length
        self.max_history_num = config.max_history_num
        self.scalar = math.sqrt(float(config.HDC_filter_num))
        self.conv_3D_a = nn.Conv3d(in_channels=4, out_channels=config.conv3D_filter_num_first, kernel_size=config.conv3D_kernel_size_first)
        self.conv_3D_b = nn.Conv3d(in_channels=config.conv3D_filter_num_first, out_channels=config.conv3D_filter_num_second,
                                   kernel_size=config.conv3D_kernel_size_second)
        self.maxpool_3D = nn.MaxPool3d(kernel_size=config.maxpooling3D_size, stride=config.maxpooling3D_stride)
        self.pool_size, self.pool_stride = int(config.maxpooling3D_size), int(config.maxpooling3D_stride)

    def initialize(self):
        pass

    def encode_user(self, history_embedding, user_history_mask, user_history_graph, user_history_category_mask,
                    user_history_category_indices, candidate_news_representation):
        from . import functional as Fn
        (h0, hL), (c0, cL) = history_embedding, candidate_news_representation
        B, H, S, E = h0.shape
        N, F = c0.shape[1], hL.shape[4]
        return Fn.FimFn.apply(c0.reshape(B * N, S, E), cL.reshape(3, B * N, S, F), h0.reshape(B * H, S, E), hL.reshape(3, B * H, S, F), self, B, N, H)
