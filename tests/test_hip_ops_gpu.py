"""GPU parity of the individual C-ABI entry points against fp64 CPU references (run with -m gpu on the MI355X box)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def close(actual, expect, tol=2e-5, what=''):
    a = actual.detach().double().cpu()
    e = expect.detach().double().cpu()
    scale = max(1.0, float(e.abs().max()))
    err = float((a - e).abs().max())
    assert err <= tol * scale, '%s: max err %.3e (scale %.3e)' % (what, err, scale)


# ------------------------------------------------------------------------------------------------ GEMM
def test_gemm_nt_bias_relu_and_unaligned():
    from nnr_amd import ops
    for (M, N, K, seed) in ((300, 225, 900, 1), (130, 900, 225, 2), (2000, 400, 300, 3), (70, 37, 50, 4)):
        x, w, b = rnd(M, K, seed=seed), rnd(N, K, seed=seed + 10), rnd(N, seed=seed + 20)
        out = ops.linear_fwd(x.to(dev()), w.to(dev()), b.to(dev()), act=ops.ACT_RELU)
        close(out, torch.relu(x.double() @ w.double().t() + b.double()), what='NT %s' % ((M, N, K),))


@pytest.mark.parametrize('tile', [2, 4, 5, 6])
def test_gemm_all_tiles_all_modes(tile):
    from nnr_amd import ops
    d = dev()
    M, N, K = 700, 300, 404
    a, b = rnd(M, K, seed=1), rnd(N, K, seed=2)
    out = torch.empty(M, N, device=d)
    ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=tile)
    close(out, a.double() @ b.double().t(), what='NT tile %d' % tile)
    bt = rnd(K, N, seed=3)
    ops.gemm(a.to(d), bt.to(d), out, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, trans_b=True, tile=tile)
    close(out, a.double() @ bt.double(), what='NN tile %d' % tile)
    at = rnd(K, M, seed=4)
    o2 = torch.zeros(M, N, device=d)
    ops.gemm(at.to(d), bt.to(d), o2, M=M, N=N, K=K, lda=M, ldb=N, ldc=N, trans_a=True, trans_b=True, split_k=3, atomic=True, tile=tile)
    close(o2, at.double().t() @ bt.double(), tol=5e-5, what='TN tile %d' % tile)


@pytest.mark.parametrize('M,N,K', [(37, 83, 70), (320, 400, 400), (3200, 200, 400), (1, 80, 64), (500, 225, 901)])
def test_gemm_skinny_tile_all_epilogues(M, N, K):
    """tile 7 (16 x 80 tiles, K split over the four waves): NT and NN, ragged sizes, unaligned leading dimensions, every
    element-wise epilogue option, batched; and the automatic choice for small launches gives the same numbers."""
    from nnr_amd import ops
    d = dev()
    a, b, bt = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(K, N, seed=3)
    bias, resid, mul, base = rnd(N, seed=4), rnd(M, N, seed=5), rnd(M, N, seed=6), rnd(M, N, seed=7)
    rv, rmap = rnd(5, N, seed=8), torch.randint(0, 5, (M,), generator=torch.Generator().manual_seed(9)).int()
    for tile in (7, 0):
        out = torch.empty(M, N, device=d)
        ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=tile)
        close(out, a.double() @ b.double().t(), what='skinny NT')
        ops.gemm(a.to(d), bt.to(d), out, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, trans_b=True, tile=tile)
        close(out, a.double() @ bt.double(), what='skinny NN')
        aux = torch.empty(M, N, device=d)
        out = base.to(d).clone()
        ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, alpha=0.5, bias=bias.to(d), rowvec=rv.to(d), ldrv=N, rowvec_map=rmap.to(d),
                 act=ops.ACT_TANH, aux_out=aux, ldaux=N, mul=mul.to(d), ldmul=N, resid=resid.to(d), ldres=N, accumulate=True, tile=tile)
        pre = torch.tanh(0.5 * (a.double() @ b.double().t()) + bias.double() + rv.double()[rmap.long()])
        close(aux, pre, what='skinny aux')
        close(out, base.double() + pre * mul.double() + resid.double(), what='skinny full epilogue')
        out = base.to(d).clone()
        ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias.to(d), act=ops.ACT_RELU, accumulate=2, tile=tile)
        close(out, torch.relu(base.double() + a.double() @ b.double().t() + bias.double()), what='skinny accumulate-before-activation')
    ab, bb = rnd(6, M, K, seed=10), rnd(6, K, N, seed=11)
    ob = torch.empty(6, M, N, device=d)
    ops.gemm(ab.to(d), bb.to(d), ob, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, trans_b=True, batch=6, strideA=M * K, strideB=K * N, strideC=M * N, tile=7)
    close(ob, ab.double() @ bb.double(), what='skinny batched NN')


PIPE_TILES = [9, 15, 16]
PIPE2_TILES = [9]


@pytest.mark.parametrize('tile', PIPE_TILES)
@pytest.mark.parametrize('M,N,K', [(37, 83, 68), (700, 300, 404), (3200, 200, 400), (1, 80, 4), (500, 228, 900), (1111, 1664, 300)])
def test_gemm_pipelined_nt_tiles(tile, M, N, K):
    """The LDS-DMA staged NT kernel (csrc/gemm.hip: gemm_nt_pipe_kernel), every tile shape: ragged M / N (rows and columns beyond
    the edge come from the zero page), K not a multiple of the stage depth (k-chunks beyond K come from the zero page), K
    shorter than one stage, fewer stages than buffers, every element-wise epilogue, dynamic M, row gather, atomic row
    scatter, batched."""
    from nnr_amd import ops
    d = dev()
    a, b = rnd(M, K, seed=1), rnd(N, K, seed=2)
    out = torch.empty(M, N, device=d)
    ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=tile)
    close(out, a.double() @ b.double().t(), what='pipe NT tile %d' % tile)
    if M < 37:
        return
    bias, resid, mul, base = rnd(N, seed=4), rnd(M, N, seed=5), rnd(M, N, seed=6), rnd(M, N, seed=7)
    rv, rmap = rnd(5, N, seed=8), torch.randint(0, 5, (M,), generator=torch.Generator().manual_seed(9)).int()
    aux = torch.empty(M, N, device=d)
    out = base.to(d).clone()
    ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, alpha=0.5, bias=bias.to(d), rowvec=rv.to(d), ldrv=N, rowvec_map=rmap.to(d),
             act=ops.ACT_TANH, aux_out=aux, ldaux=N, mul=mul.to(d), ldmul=N, resid=resid.to(d), ldres=N, accumulate=True, tile=tile)
    pre = torch.tanh(0.5 * (a.double() @ b.double().t()) + bias.double() + rv.double()[rmap.long()])
    etol = 2e-5 * max(1.0, math.sqrt(K / 100.0))          # the pre-activation is an fp32 sum of K products of magnitude ~1
    close(aux, pre, tol=etol, what='pipe aux')
    close(out, base.double() + pre * mul.double() + resid.double(), tol=etol, what='pipe full epilogue')
    # dynamic M + row gather (negative index = zero row) + rows beyond the live count untouched
    used = max(1, (M * 2) // 3)
    V = 97
    tab = rnd(V, K, seed=11)
    idx = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(12)).int()
    idx[min(5, used - 1)] = -1
    out = torch.full((M, N), 7.0, device=d)
    dyn = torch.tensor([used], dtype=torch.int32, device=d)
    if tile in PIPE2_TILES:                                 # the gen-2 loop takes no row gather: dynamic M only
        ops.gemm(a.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, dyn=dyn, dyn_dim=1, bias=bias.to(d), tile=tile)
        exp = a.double() @ b.double().t() + bias.double()
    else:
        ops.gemm(tab.to(d), b.to(d), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, a_idx=idx.to(d), dyn=dyn, dyn_dim=1, bias=bias.to(d), tile=tile)
        g = tab.double()[idx.long().clamp_min(0)] * (idx >= 0).double()[:, None]
        exp = g @ b.double().t() + bias.double()
    close(out[:used], exp[:used], what='pipe gather dyn')
    assert bool((out[used:] == 7.0).all())
    # atomic row scatter (embedding-gradient shape): C[c_idx[m]] += row m
    rows = 50
    cidx = torch.randint(0, rows, (M,), generator=torch.Generator().manual_seed(13)).int()
    cidx[0] = -1
    acc = torch.zeros(rows, N, device=d)
    ops.gemm(a.to(d), b.to(d), acc, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, c_idx=cidx.to(d), atomic=True, tile=tile)
    full = a.double() @ b.double().t()
    exp = torch.zeros(rows, N, dtype=torch.double)
    keep = cidx >= 0
    exp.index_add_(0, cidx[keep].long(), full[keep])
    close(acc, exp, tol=5e-5, what='pipe scatter')
    if M <= 700:
        ab, bb = rnd(3, M, K, seed=20), rnd(3, N, K, seed=21)
        ob = torch.empty(3, M, N, device=d)
        ops.gemm(ab.to(d), bb.to(d), ob, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, batch=3, strideA=M * K, strideB=N * K, strideC=M * N, tile=tile)
        close(ob, ab.double() @ bb.double().transpose(1, 2), what='pipe batched')


@pytest.mark.parametrize('M,N,K', [(70000, 400, 400), (33000, 1664, 300), (5000, 200, 200), (4352, 900, 900), (300, 84, 96), (129, 400, 104), (2500, 300, 1664)])
def test_gemm_bf16x3_tile(M, N, K):
    """Tile 50 (csrc/gemm.hip: gemm_nt_bx3_kernel; the default matrix path of weight-operand NT launches since round 6, NNR_BX3=0 turns it off): the NT product on the BF16 matrix pipe as six exact
    bf16 x bf16 products with fp32 accumulation, weights pre-split by nnr_split_bf16x3.  The split is EXACT (w == image0 + image1 + image2 bit for
    bit), the product is at least as close to fp64 as the fp32-MFMA kernel's, and every element-wise epilogue / dynamic M / k-tail / ragged
    edge behaves as in the other NT kernels."""
    from nnr_amd import ops
    d = dev()
    a, b = rnd(M, K, seed=1).to(d), rnd(N, K, seed=2, scale=0.2).to(d)
    img, stride, ldo = ops.bx3_images(b, N, K, K)
    bf = img.view(torch.bfloat16).float()                       # [3, N, ldo]
    assert ldo % 8 == 0 and ldo >= K and torch.equal((bf[0] + bf[1]) + bf[2], torch.nn.functional.pad(b, (0, ldo - K)))
    b3 = (img, stride, ldo)
    full = a.cpu().double() @ b.cpu().double().t()
    out, ref = torch.empty(M, N, device=d), torch.empty(M, N, device=d)
    ops.gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=50, b3=b3)
    ops.gemm(a, b, ref, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=15)
    e50 = float((out.cpu().double() - full).norm() / full.norm())
    e15 = float((ref.cpu().double() - full).norm() / full.norm())
    assert e50 <= 1.05 * e15 + 1e-9, (e50, e15)
    etol = 2e-5 * max(1.0, math.sqrt(K / 100.0))
    close(out, full, tol=etol, what='bx3 plain')
    bias, resid, mul, base = rnd(N, seed=4).to(d), rnd(M, N, seed=5).to(d), rnd(M, N, seed=6).to(d), rnd(M, N, seed=7).to(d)
    rv, rmap = rnd(5, N, seed=8).to(d), torch.randint(0, 5, (M,), generator=torch.Generator().manual_seed(9)).int().to(d)
    aux = torch.empty(M, N, device=d)
    out = base.clone()
    ops.gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, alpha=0.5, bias=bias, rowvec=rv, ldrv=N, rowvec_map=rmap, act=ops.ACT_TANH, aux_out=aux, ldaux=N,
             mul=mul, ldmul=N, resid=resid, ldres=N, accumulate=True, tile=50, b3=b3)
    pre = torch.tanh(0.5 * full + bias.cpu().double() + rv.cpu().double()[rmap.cpu().long()])
    close(aux, pre, tol=etol, what='bx3 aux')
    close(out, base.cpu().double() + pre * mul.cpu().double() + resid.cpu().double(), tol=etol, what='bx3 full epilogue')
    used = max(1, (M * 2) // 3)
    out = torch.full((M, N), 7.0, device=d)
    dyn = torch.tensor([used], dtype=torch.int32, device=d)
    ops.gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, dyn=dyn, dyn_dim=1, bias=bias, tile=50, b3=b3)
    close(out[:used], (full + bias.cpu().double())[:used], tol=etol, what='bx3 dyn')
    assert bool((out[used:] == 7.0).all())
    with pytest.raises(Exception):                              # without the pre-split weights the tile is refused
        ops.gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=50)


def test_gemm_bf16x3_edge_values():
    """The bf16x3 matrix path (default since round 6) on inputs a normal(0, sigma) test never produces (round-5 verdict):
      * magnitudes mixed over 1e-20 .. 1e20 inside one dot product;  * catastrophic cancellation (pairs +x, -x (1 - 2^-20): the sum is 2^-20 of the
        terms);  * fp32 denormals (bits below bf16's smallest subnormal 2^-133 underflow: absolute error <= 2^-133 per operand);  * values at and next to FLT_MAX (a bf16 ROUNDING of them is +-Inf: the split truncates there and stays exact);
      * +-Inf / NaN: every output they reach is non-finite (+-Inf or NaN), every other output is untouched -- non-finite never becomes finite.
    Error measure: |got - fp64| <= bound x sum_k |a_k b_k| (the forward error bound of any dot product), with the fp32-MFMA kernel as the yardstick."""
    from nnr_amd import ops
    d = dev()
    M, N, K = 4096, 160, 256
    g = torch.Generator().manual_seed(11)

    def run(a, b, tile_ref=15):
        a, b = a.to(d).contiguous(), b.to(d).contiguous()
        img, stride, ldo = ops.bx3_images(b, N, K, K)
        bf = img.view(torch.bfloat16).double()                     # (summed in fp64: FLT_MAX = 0x7F7F0000 + 2^120 - 2^104 passes through 2^128 in fp32)
        # exact wherever all three images are representable: |w| >= 2^-109 (the third image's last bit is 2^-24 |w| and bf16's smallest
        # subnormal is 2^-133); below that the bits under 2^-133 underflow: absolute error <= 2^-133, a 1e5-th of fp32's smallest NORMAL value
        rebuilt = ((bf[0] + bf[1]) + bf[2])[:, :K]
        normal = torch.isfinite(b) & ((b.abs() >= 2.0 ** -109) | (b == 0))
        assert torch.equal(rebuilt[normal], b[normal].double()), 'the split of a finite fp32 value >= 2^-109 must be exact'
        tiny = torch.isfinite(b) & ~normal
        if bool(tiny.any()):
            assert float((rebuilt[tiny] - b[tiny].double()).abs().max()) <= 2.0 ** -133
        out, ref = torch.empty(M, N, device=d), torch.empty(M, N, device=d)
        ops.gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=50, b3=(img, stride, ldo))
        ops.gemm(a, b, ref, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, tile=tile_ref)
        return out.cpu().double(), ref.cpu().double()

    def check(a, b, what):
        out, ref = run(a, b)
        full = a.double() @ b.double().t()
        scale = a.double().abs() @ b.double().abs().t()
        e50 = float(((out - full).abs() / scale.clamp_min(1e-300)).max())
        e15 = float(((ref - full).abs() / scale.clamp_min(1e-300)).max())
        assert bool(torch.isfinite(out).all()), what
        assert e50 <= max(1.05 * e15, 2.0 ** -22), (what, e50, e15)        # (2^-22: a few fp32 roundings of the accumulated sum)
        return e50, e15

    # 1. mixed magnitudes: exponents uniform over +-20 decades, per element
    a = torch.randn(M, K, generator=g) * 10.0 ** (torch.rand(M, K, generator=g) * 40 - 20)
    b = torch.randn(N, K, generator=g) * 10.0 ** (torch.rand(N, K, generator=g) * 30 - 15)
    check(a, b, 'mixed magnitudes')
    # 2. catastrophic cancellation: columns 2j, 2j + 1 hold +x and -x (1 - 2^-20) against equal weights
    x = torch.randn(M, K // 2, generator=g)
    a = torch.stack([x, -x * (1 - 2.0 ** -20)], dim=2).reshape(M, K)
    w = torch.randn(N, K // 2, generator=g)
    b = torch.stack([w, w], dim=2).reshape(N, K)
    e50, e15 = check(a, b, 'cancellation')
    out, _ = run(a, b)
    full = a.double() @ b.double().t()
    assert float((out - full).norm() / full.norm()) <= 2e-2          # the RESULT (2^-20 of the terms) still has ~6 of its bits right in fp32 arithmetic
    # 3. denormals (and a few normal values so the result is not all-zero)
    a = torch.randn(M, K, generator=g) * 1e-39
    a[:, ::7] = torch.randn(M, (K + 6) // 7, generator=g)
    b = torch.randn(N, K, generator=g)
    b[:, 1::5] *= 1e-40
    check(a, b, 'denormals')
    # 4. at and next to FLT_MAX: one huge value per row against weights <= 2^-8 so that the exact result stays finite
    big = torch.tensor([3.4028234663852886e38, 3.3895313892515355e38, 3.3961775292304325e38, -3.4028234663852886e38])      # FLT_MAX, bf16 max, bf16 max + half ulp, -FLT_MAX
    a = torch.randn(M, K, generator=g)
    a[:, 3] = big[torch.arange(M) % 4]
    b = torch.randn(N, K, generator=g) * 2.0 ** -9
    check(a, b, 'near FLT_MAX')
    # ... and huge WEIGHTS (the pre-split side)
    a = torch.randn(M, K, generator=g) * 2.0 ** -9
    b = torch.randn(N, K, generator=g)
    b[:, 5] = big[torch.arange(N) % 4]
    check(a, b, 'near FLT_MAX weights')
    # 5. non-finite: rows 0 / 1 / 2 of A carry +Inf / -Inf / NaN, column 7 of the weights carries +Inf in row 3
    a = torch.randn(M, K, generator=g)
    b = torch.randn(N, K, generator=g)
    a[0, 10], a[1, 11], a[2, 12] = float('inf'), float('-inf'), float('nan')
    b[3, 7] = float('inf')
    out, ref = run(a, b)
    bad = torch.zeros(M, N, dtype=torch.bool)
    bad[:3, :] = True
    bad[:, 3] = True
    assert not bool(torch.isfinite(out[bad]).any()), 'a non-finite operand must give a non-finite value in every output it reaches'
    assert not bool(torch.isfinite(ref[bad]).any())                  # (the fp32-MFMA kernel: +-Inf or NaN there)
    full = torch.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0).double() @ torch.nan_to_num(b, posinf=0.0).double().t()
    assert bool(torch.isfinite(out[~bad]).all()) and float((out[~bad] - full[~bad]).abs().max()) <= 1e-4


def test_gemm_nn_accumulate_and_tn_splitk_dyn():
    from nnr_amd import ops
    dy, w = rnd(300, 225, seed=1), rnd(225, 900, seed=2)
    base = rnd(300, 900, seed=3)
    out = base.to(dev()).clone()
    ops.linear_bwd_data(dy.to(dev()), w.to(dev()), out=out, accumulate=True)
    close(out, base.double() + dy.double() @ w.double(), what='NN accumulate')
    R, used = 5000, 3777
    dy, x = rnd(R, 832, seed=4), rnd(R, 300, seed=5)
    dw = torch.zeros(832, 300, device=dev())
    dyn = torch.tensor([used], dtype=torch.int32, device=dev())
    ops.linear_bwd_weight(dy.to(dev()), x.to(dev()), dw, dyn=dyn)
    close(dw, dy[:used].double().t() @ x[:used].double(), tol=5e-5, what='TN split-K dyn')


def test_gemm_gather_rowdot_gate_batched():
    from nnr_amd import ops
    d = dev()
    # gather + dyn M + bias (LSTM input projection shape)
    V, E, NP2, cap, used = 1000, 300, 1664, 5000, 4321
    emb, w, b = rnd(V, E, seed=1), rnd(NP2, E, seed=2, scale=0.1), rnd(NP2, seed=3)
    idx = torch.randint(0, V, (cap,), generator=torch.Generator().manual_seed(4)).int()
    idx[17] = -1
    out = torch.full((cap, NP2), 7.0, device=d)
    dyn = torch.tensor([used], dtype=torch.int32, device=d)
    ops.gemm(emb.to(d), w.to(d), out, M=cap, N=NP2, K=E, lda=E, ldb=E, ldc=NP2, a_idx=idx.to(d), dyn=dyn, dyn_dim=1, bias=b.to(d))
    x = emb[idx.clamp_min(0).long()].double()
    x[17] = 0
    ref = x @ w.double().t() + b.double()
    close(out[:used], ref[:used], what='gather GEMM')
    assert float((out[used:] - 7.0).abs().max()) == 0.0, 'rows past the dynamic extent must not be written'
    # fused tanh . w2 row-dot (tile 3)
    M, F, A = 1000, 400, 200
    x, w1, b1, w2 = rnd(M, F, seed=5), rnd(A, F, seed=6, scale=0.05), rnd(A, seed=7, scale=0.1), rnd(1, A, seed=8)
    th = torch.empty(M, A, device=d)
    sc = torch.empty(M, device=d)
    ops.gemm(x.to(d), w1.to(d), None, M=M, N=A, K=F, lda=F, ldb=F, bias=b1.to(d), act=ops.ACT_TANH, aux_out=th, ldaux=A,
             rowdot_w=w2.to(d), rowdot_out=sc, tile=3)
    tref = torch.tanh(x.double() @ w1.double().t() + b1.double())
    close(th, tref, what='tanh aux')
    close(sc, tref @ w2.double()[0], what='rowdot')
    # gate epilogue: h * sigmoid(h W^T + P[map])
    M, F, n = 900, 400, 40
    h, w, P = rnd(M, F, seed=9), rnd(F, F, seed=10, scale=0.05), rnd(n, F, seed=11)
    rmap = torch.randint(0, n, (M,), generator=torch.Generator().manual_seed(12)).int()
    G = torch.empty(M, F, device=d)
    Ht = torch.empty(M, F, device=d)
    hd = h.to(d)
    ops.gemm(hd, w.to(d), Ht, M=M, N=F, K=F, lda=F, ldb=F, ldc=F, rowvec=P.to(d), ldrv=F, rowvec_map=rmap.to(d), act=ops.ACT_SIGMOID,
             aux_out=G, ldaux=F, mul=hd, ldmul=F)
    gref = torch.sigmoid(h.double() @ w.double().t() + P.double()[rmap.long()])
    close(G, gref, what='gate G')
    close(Ht, gref * h.double(), what='gate Ht')
    # batched 68x68 aggregate with bias / relu / residual
    Bt, Gn, D = 5, 68, 900
    graph, z, bias, xres = rnd(Bt, Gn, Gn, seed=13, scale=0.2), rnd(Bt, Gn, D, seed=14), rnd(D, seed=15), rnd(Bt, Gn, D, seed=16)
    y = torch.empty(Bt, Gn, D, device=d)
    r = torch.empty(Bt, Gn, D, device=d)
    ops.gemm(graph.to(d), z.to(d), y, M=Gn, N=D, K=Gn, lda=Gn, ldb=D, ldc=D, trans_b=True, bias=bias.to(d), act=ops.ACT_RELU, aux_out=r,
             ldaux=D, resid=xres.to(d), ldres=D, batch=Bt, strideA=Gn * Gn, strideB=Gn * D, strideC=Gn * D, stride_aux=Gn * D,
             stride_res=Gn * D, tile=2)
    rref = torch.relu(torch.einsum('bij,bjd->bid', graph.double(), z.double()) + bias.double())
    close(r, rref, what='batched relu aux')
    close(y, rref + xres.double(), what='batched + residual')
    # A^T (graph transpose) batched
    dz = torch.empty(Bt, Gn, D, device=d)
    ops.gemm(graph.to(d), z.to(d), dz, M=Gn, N=D, K=Gn, lda=Gn, ldb=D, ldc=D, trans_a=True, trans_b=True, batch=Bt, strideA=Gn * Gn,
             strideB=Gn * D, strideC=Gn * D, tile=2)
    close(dz, torch.einsum('bij,bid->bjd', graph.double(), z.double()), what='batched A^T')


def test_gemm_dropout_masks_are_consistent():
    """The same (seed, row, col) mask must be seen by the forward gather (target 1), the weight-gradient B loader
    (target 2) and the scatter epilogue (target 4)."""
    from nnr_amd import ops
    d = dev()
    V, E, R, p, seed = 50, 300, 700, 0.3, 1234
    emb = (rnd(V, E, seed=1).abs() + 0.5).to(d)
    idx = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(2)).int().to(d)
    eye = torch.eye(E, device=d)
    xd = torch.empty(R, E, device=d)
    ops.gemm(emb, eye, xd, M=R, N=E, K=E, lda=E, ldb=E, ldc=E, a_idx=idx, drop=(1, p, seed, E))       # = dropout(emb[idx])
    x = emb[idx.long()]
    keep = xd != 0
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) < 0.02, frac
    close(xd, torch.where(keep, x / (1 - p), torch.zeros_like(x)), what='dropout scale')
    dy = rnd(R, 64, seed=3).to(d)
    dw = torch.zeros(64, E, device=d)
    ops.gemm(dy, emb, dw, M=64, N=E, K=R, lda=64, ldb=E, ldc=E, trans_a=True, trans_b=True, b_idx=idx, drop=(2, p, seed, E), split_k=4,
             atomic=True)
    close(dw, dy.double().t().cpu() @ xd.double().cpu(), tol=5e-5, what='target-2 mask')
    dtab = torch.zeros(V, E, device=d)
    ones = torch.ones(R, E, device=d)
    ops.gemm(ones, eye, dtab, M=R, N=E, K=E, lda=E, ldb=E, ldc=E, trans_b=True, c_idx=idx, atomic=True, drop=(4, p, seed, E))
    ref = torch.zeros(V, E, dtype=torch.float64)
    ref.index_add_(0, idx.long().cpu(), keep.double().cpu() / (1 - p))
    close(dtab, ref, what='target-4 scatter mask')


# ------------------------------------------------------------------------------------------------ planner + LSTM
def _lengths(n, Lx, seed):
    g = torch.Generator().manual_seed(seed)
    l = torch.randint(1, Lx + 1, (n,), generator=g)
    l[0] = Lx
    l[1] = 1
    return l


def test_seq_plan_matches_stable_sort():
    from nnr_amd import ops
    n, Lx = 333, 32
    lens = _lengths(n, Lx, 5)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    mask[7] = False            # an all-false row: position 0 must be forced on (newsEncoders.py:108)
    lens[7] = 1
    ids = torch.randint(2, 1000, (n, Lx), generator=torch.Generator().manual_seed(6)).int() * mask.int()
    md = mask.clone().to(dev())
    plan = ops.SeqPlan(md, ids.to(dev()))
    order = torch.argsort(lens, descending=True, stable=True)
    assert bool(md[7, 0]) and int(md.sum()) == int(lens.sum())
    assert torch.equal(plan.order.cpu().long(), order)
    assert torch.equal(plan.slen.cpu().long(), lens[order])
    bs = torch.tensor([(lens > t).sum() for t in range(Lx)])
    assert torch.equal(plan.bs.cpu().long(), bs)
    off = torch.cat([torch.zeros(1, dtype=torch.long), bs.cumsum(0)])
    assert torch.equal(plan.off.cpu().long(), off)
    tok, rs, pf, pr = plan.tok.cpu(), plan.row_seq.cpu(), plan.prev_f.cpu(), plan.prev_r.cpu()
    for s in (0, 1, 50, n - 1):
        i = int(order[s])
        for t in range(int(lens[i])):
            row = int(off[t]) + s
            assert int(tok[row]) == int(ids[i, t]) and int(rs[row]) == s
            assert int(pf[row]) == (int(off[t - 1]) + s if t > 0 else -1)
            assert int(pr[row]) == (int(off[t + 1]) + s if t + 1 < int(lens[i]) else -1)
    # caller-supplied order
    perm = torch.sort(lens, descending=True)[1].int()
    plan2 = ops.SeqPlan(mask.clone().to(dev()), ids.to(dev()), perm.to(dev()))
    assert torch.equal(plan2.order.cpu(), perm)


@pytest.mark.parametrize('n0,n1', [(37, 203), (320, 3200), (5, 1)])
def test_seq_plan_pair_and_per_call_rank_pairing(n0, n1):
    """Two encoder calls planned as one packed stream: the union plan equals the plan of the concatenated inputs, both masks
    get the mask[:,0]=1 fix, and nnr_cne_pair_map pairs title position r of a call with content position r of the SAME call
    (newsEncoders.py:112-115,128-129 applied per call)."""
    from nnr_amd import ops
    n = n0 + n1
    Lt, Lc = 12, 40
    lt, lc = _lengths(n, Lt, 11), _lengths(n, Lc, 12)
    mt = torch.arange(Lt)[None, :] < lt[:, None]
    mt[3] = False
    lt[3] = 1
    ids = torch.randint(2, 1000, (n, Lt), generator=torch.Generator().manual_seed(13)).int() * mt.int()
    m0, m1 = mt[:n0].clone().to(dev()), mt[n0:].clone().to(dev())
    plan_t = ops.SeqPlan(m0, ids[:n0].contiguous().to(dev()), None, m1, ids[n0:].contiguous().to(dev()))
    ref = ops.SeqPlan(mt.clone().to(dev()), ids.to(dev()))
    for k in ('len', 'order', 'rank', 'slen', 'bs', 'off'):
        assert torch.equal(getattr(plan_t, k), getattr(ref, k)), k
    tot = int(plan_t.off[-1])
    for k in ('row_seq', 'tok', 'prev_f', 'prev_r'):
        assert torch.equal(getattr(plan_t, k)[:tot], getattr(ref, k)[:tot]), k
    assert bool(m0[3, 0]) and int(m0.sum()) + int(m1.sum()) == int(lt.sum())
    mc = torch.arange(Lc)[None, :] < lc[:, None]
    plan_c = ops.SeqPlan(mc[:n0].clone().to(dev()), None, None, mc[n0:].clone().to(dev()), None)
    pm_t, pm_c = [x.cpu().long() for x in ops.cne_pair_map(plan_t, plan_c)]
    # expected: per call, stable descending order of each stream; partner of title position r = content position r
    rank_t, rank_c = plan_t.rank.cpu().long(), plan_c.rank.cpu().long()
    exp_t = torch.empty(n, dtype=torch.long)
    for lo, hi in ((0, n0), (n0, n)):
        ot = torch.argsort(lt[lo:hi], descending=True, stable=True) + lo
        oc = torch.argsort(lc[lo:hi], descending=True, stable=True) + lo
        exp_t[rank_t[ot]] = rank_c[oc]
    assert torch.equal(pm_t, exp_t)
    assert torch.equal(pm_c[pm_t], torch.arange(n))


def test_seq_plan_long_sequences_take_the_small_lds_path():
    """L = 512 with n near 8 192: the fast ranking's per-segment histograms (128 x 513 ints = 263 KB) exceed the 160 KB of LDS; the
    planner must fall back to the ranking that needs 2 * (L + 1) ints instead of refusing the call (ADVICE, round 1)."""
    from nnr_amd import ops
    n, Lx = 8000, 512
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, Lx + 1, (n,), generator=g)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    plan = ops.SeqPlan(mask.clone().to(dev()), None)
    order = torch.argsort(lens, descending=True, stable=True)
    assert torch.equal(plan.order.cpu().long(), order)
    assert torch.equal(plan.slen.cpu().long(), lens[order])
    assert int(plan.off.cpu()[-1]) == int(lens.sum())


def test_pair_recurrence_timeout_is_counted_and_skips_the_optimizer(monkeypatch):
    """The CU-pair exchange must fail LOUDLY: with the tagged stores switched off (debug bit 2 of NNR_LSTM_DBG) every partner
    wait runs into its bound, the per-launch diagnostics word AND the persistent counter become non-zero, h is poisoned with
    NaN, and clip+Adam leaves parameters and moments untouched for a gradient whose norm is not finite."""
    from nnr_amd import ops
    from nnr_amd.layers import LSTMParams
    monkeypatch.setattr(ops, 'LSTM_PAIR', True)
    d = dev()
    n, Lx, E, H = 32, 6, 300, 200
    lens = torch.full((n,), Lx)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    ids = torch.arange(n * Lx, dtype=torch.int32).view(n, Lx)
    plan = ops.SeqPlan(mask.clone().to(d), ids.to(d))
    holder = LSTMParams(E, H).to(d)
    w = ops.LstmPacked(holder.param_list(), H, E)
    f32 = dict(device=d, dtype=torch.float32)
    cap = plan.cap
    st = dict(plan=plan, w=w, gates=torch.randn((cap, 2 * w.NP), **f32) * 0.1, cell=torch.empty((cap, 2 * w.HP), **f32),
              hout=torch.zeros((cap, 2 * H), **f32), cn=torch.empty((n, 2 * H), **f32))
    ops.lstm_sync_timeouts(reset=True)
    ops.lstm_fwd([st], H)
    torch.cuda.synchronize()
    assert ops.lstm_sync_timeouts() == 0 and ops.lstm_last_launch_timeouts() == 0 and bool(torch.isfinite(st['hout']).all())
    monkeypatch.setenv('NNR_LSTM_DBG', '2')
    ops.lstm_fwd([st], H)
    torch.cuda.synchronize()
    monkeypatch.delenv('NNR_LSTM_DBG')
    assert ops.lstm_last_launch_timeouts() > 0
    total = ops.lstm_sync_timeouts()
    assert total > 0 and not bool(torch.isfinite(st['hout']).all())
    ops.lstm_fwd([st], H)                                   # a clean launch: its own diagnostics are 0, the total stays
    torch.cuda.synchronize()
    assert ops.lstm_last_launch_timeouts() == 0 and ops.lstm_sync_timeouts(reset=True) == total and ops.lstm_sync_timeouts() == 0
    # the poisoned step never reaches the parameters
    p = torch.randn(1000, **f32); g = torch.randn(1000, **f32); g[7] = float('nan')
    m = torch.zeros(1000, **f32); v = torch.zeros(1000, **f32); ss = torch.zeros(1, **f32)
    p0 = p.clone()
    ops.sumsq(g, ss)
    ops.clip_adam(p, g, m, v, ss, 1.0, 4.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert torch.equal(p, p0) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


@pytest.mark.parametrize('n,Lx,E,H,variant', [(37, 12, 16, 8, 'one'), (100, 32, 300, 200, 'one'), (45, 128, 300, 200, 'one'),
                                              (100, 32, 300, 200, 'pair'), (45, 128, 300, 200, 'pair'), (200, 128, 300, 200, 'pair'),
                                              (45, 128, 300, 200, 'pair_fabric'), (45, 128, 300, 200, 'pair_noquad'),
                                              (203, 40, 300, 200, 'pair_quad6'), (45, 128, 300, 200, 'pair_quad20'),
                                              (1100, 24, 300, 200, 'pair_quad3'), (45, 128, 300, 200, 'pair_fabric_quad20'),
                                              (200, 32, 300, 200, 'pair_ones'), (90, 40, 300, 200, 'pair_quad6_ones')])
def test_bilstm_forward_backward_matches_oracle(n, Lx, E, H, variant, monkeypatch):
    """'one': one workgroup per 16-sequence tile (W_hh streamed from L2);  'pair': two workgroups on two CUs of one XCD with
    W_hh resident, exchanging through that XCD's L2 (sequences longer than 64 steps in 4-row tiles);  'pair_fabric': the same with
    the cross-XCD (write-through) exchange flavour forced -- the fallback the kernel takes when the placement handshake finds the
    halves on different XCDs;  'pair_noquad' / 'pair_quadT': 4-row tiles off / for every sequence longer than T steps (T = 3 with
    1 100 sequences: more long sequences than the 64 quad tiles hold, the rest stay in 16-row tiles)."""
    from nnr_amd import ops
    from nnr_amd.layers import LSTMParams
    from oracle.nnr_oracle import BiLSTM
    monkeypatch.setattr(ops, 'LSTM_PAIR', variant != 'one')
    if 'fabric' in variant:
        monkeypatch.setenv('NNR_LSTM_DBG', '64')
    if variant == 'pair_noquad':
        monkeypatch.setenv('NNR_LSTM_QUAD_T', '0')
    if 'quad' in variant and variant != 'pair_noquad':
        monkeypatch.setenv('NNR_LSTM_QUAD_T', variant.split('quad')[1].split('_')[0])
    d = dev()
    torch.manual_seed(n)
    lens = _lengths(n, Lx, n)
    if variant.endswith('ones'):
        lens[n // 3:] = 1          # padded history slots: whole tiles of one-token sequences take the element-wise path of the pair kernels
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    x = rnd(n, Lx, E, seed=1, scale=0.5)
    ref = BiLSTM(E, H).double()
    with torch.no_grad():
        for q in ref.parameters():
            q.mul_(1.5)
    holder = LSTMParams(E, H)
    holder.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    holder = holder.to(d)
    # reference forward / backward in fp64
    xr = x.double().requires_grad_(True)
    Hr, cr = ref(xr, lens)
    dH = rnd(n, Lx, 2 * H, seed=2) * mask[:, :, None]
    dc = rnd(n, 2 * H, seed=3)
    ((Hr * dH.double()).sum() + (cr * dc.double()).sum()).backward()
    # HIP path: table = flattened x, ids = arange
    ids = torch.arange(n * Lx, dtype=torch.int32).view(n, Lx)
    plan = ops.SeqPlan(mask.clone().to(d), ids.to(d))
    w = ops.LstmPacked(holder.param_list(), H, E)
    table = x.view(n * Lx, E).to(d)
    cap = plan.cap
    f32 = dict(device=d, dtype=torch.float32)
    st = dict(plan=plan, w=w, gates=torch.empty((cap, 2 * w.NP), **f32), cell=torch.empty((cap, 2 * w.HP), **f32),
              hout=torch.zeros((cap, 2 * H), **f32), cn=torch.empty((n, 2 * H), **f32))
    ops.gemm(table, w.w_ihp, st['gates'], M=cap, N=2 * w.NP, K=E, lda=E, ldb=E, ldc=2 * w.NP, a_idx=plan.tok, dyn=plan.total, dyn_dim=1,
             bias=w.b_p)
    ops.lstm_fwd([st], H)
    assert ('sync' in st) == (variant != 'one') and ops.lstm_sync_timeouts() == 0
    off, rank, order = plan.off.cpu().long(), plan.rank.cpu().long(), plan.order.cpu().long()
    rows = (off[:Lx][None, :] + rank[:, None])                      # packed row of (i, t)
    hout = st['hout'].cpu()
    got = torch.where(mask[:, :, None], hout[rows.clamp_max(cap - 1)], torch.zeros(1))
    close(got, Hr, what='LSTM H')
    close(st['cn'].cpu()[rank], cr, what='LSTM c_n')
    # backward
    dh_packed = torch.zeros((cap, 2 * H))
    dh_packed[rows[mask]] = dH[mask]
    st['dh'] = dh_packed.to(d)
    st['dcn'] = dc[order].contiguous().to(d)
    ops.lstm_bwd([st], H)
    assert ops.lstm_sync_timeouts() == 0
    dg = st['gates']
    NP = w.NP
    dw_ihp = torch.zeros((2 * NP, E), **f32)
    db_p = torch.zeros(2 * NP, **f32)
    dw_hhp = torch.zeros((2, NP, H), **f32)
    ops.gemm(dg, table, dw_ihp, M=2 * NP, N=E, K=cap, lda=2 * NP, ldb=E, ldc=E, trans_a=True, trans_b=True, b_idx=plan.tok,
             split_k=ops.split_for(2 * NP, E, cap), atomic=True, dyn=plan.total, dyn_dim=2)
    ops.bias_grad(dg, db_p, dyn=plan.total, rows=cap)
    for dd, prev in ((0, plan.prev_f), (1, plan.prev_r)):
        ops.gemm(dg[:, dd * NP:], st['hout'][:, dd * H:], dw_hhp[dd], M=NP, N=H, K=cap, lda=2 * NP, ldb=2 * H, ldc=H, trans_a=True,
                 trans_b=True, b_idx=prev, split_k=ops.split_for(NP, H, cap), atomic=True, dyn=plan.total, dyn_dim=2)
    grads = [torch.zeros_like(q) for q in holder.param_list()]
    ops.lstm_unpack_grads(dw_ihp, db_p, dw_hhp, H, E, grads)
    # the consuming form (persistent workspace): same gradients, packed buffers handed back all-zero incl. the padded gate columns
    grads2 = [torch.zeros_like(q) for q in holder.param_list()]
    ops.lstm_unpack_grads(dw_ihp, db_p, dw_hhp, H, E, grads2, zero_src=True)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert float(dw_ihp.abs().max()) == 0.0 and float(db_p.abs().max()) == 0.0 and float(dw_hhp.abs().max()) == 0.0
    names = ['weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0']
    names = names + [k + '_reverse' for k in names]
    for k, g in zip(names, grads):
        close(g, getattr(ref, k).grad, tol=1e-4, what='LSTM d' + k)
    dtab = torch.zeros((n * Lx, E), **f32)
    ops.gemm(dg, w.w_ihp, dtab, M=cap, N=E, K=2 * NP, lda=2 * NP, ldb=E, ldc=E, trans_b=True, c_idx=plan.tok, atomic=True, dyn=plan.total,
             dyn_dim=1)
    close(dtab.view(n, Lx, E), xr.grad, tol=1e-4, what='LSTM dX')


# ------------------------------------------------------------------------------------------------ pools
def _softmax_pool_ref(x, score, mask):
    s = score if mask is None else torch.where(mask, score, torch.full_like(score, -1e9))
    a = torch.softmax(s, dim=1)
    return torch.einsum('nl,nld->nd', a, x), a


@pytest.mark.parametrize('quad_T', ['0', '16'])
def test_pair_recurrence_makes_progress_beside_a_cu_saturating_kernel(quad_T, monkeypatch):
    """The CU-pair recurrence spins on its partner workgroup.  Its forward-progress argument (a waiting workgroup's partner is the
    next one of ITS launch to get a CU; every wait is bounded and counted) must hold when another HIP stream keeps every CU busy:
    a stream of GPU-filling GEMM launches (the 128 x 80 LDS-DMA tile, 4 workgroups per CU) runs before, during and after the
    forward and the backward recurrence of 1 600 sequences (200 pair tiles, 1.5 x the 128 pair slots of the chip) on a second
    stream.  No exchange time-out, and bit-identical results to the same launches on an idle GPU."""
    from nnr_amd import ops
    from nnr_amd.layers import LSTMParams
    monkeypatch.setenv('NNR_LSTM_QUAD_T', quad_T)
    d = dev()
    n, Lx, E, H = 1600, 48, 300, 200
    lens = _lengths(n, Lx, 21)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    plan = ops.SeqPlan(mask.clone().to(d), None)
    holder = LSTMParams(E, H).to(d)
    torch.manual_seed(5)
    with torch.no_grad():
        for q in holder.parameters():
            q.normal_(0, 0.08)
    w = ops.LstmPacked(holder.param_list(), H, E)
    cap = plan.cap
    f32 = dict(device=d, dtype=torch.float32)
    xw = torch.randn((cap, 2 * w.NP), **f32) * 0.5
    dh = torch.randn((cap, 2 * H), **f32) * 0.1
    dcn = torch.randn((n, 2 * H), **f32) * 0.1
    A = torch.randn((65536, 512), **f32)
    Bm = torch.randn((800, 512), **f32) * 0.05
    Cm = torch.empty((65536, 800), **f32)

    def run(busy):
        st = dict(plan=plan, w=w, gates=xw.clone(), cell=torch.empty((cap, 2 * w.HP), **f32), hout=torch.zeros((cap, 2 * H), **f32),
                  cn=torch.empty((n, 2 * H), **f32), dh=dh, dcn=dcn)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=d)
        if busy:
            with torch.cuda.stream(side):
                for _ in range(24):           # ~0.5 ms each: the chip stays full for the whole recurrence (and beyond)
                    ops.gemm(A, Bm, Cm, M=65536, N=800, K=512, lda=512, ldb=512, ldc=800, tile=15)
        ops.lstm_fwd([st], H)
        fwd = (st['hout'].clone(), st['cn'].clone())
        ops.lstm_bwd([st], H)
        torch.cuda.synchronize()
        return fwd + (st['gates'].clone(),)

    ops.lstm_sync_timeouts(reset=True)
    quiet = run(False)
    loaded = run(True)
    assert ops.lstm_sync_timeouts() == 0
    for a, b, what in zip(quiet, loaded, ('h', 'c_n', 'dgates')):
        tot = int(plan.off[-1])
        a, b = (a[:tot], b[:tot]) if a.shape[0] == cap else (a, b)
        assert torch.isfinite(b).all() and torch.equal(a, b), what


@pytest.mark.parametrize('B,G,D', [(5, 68, 900), (3, 21, 52), (2, 128, 64), (4, 16, 20), (3, 50, 132), (2, 66, 900), (2, 80, 72), (3, 5, 64)])
def test_gcn_aggregate_forward_backward(B, G, D):
    """Per-user graph aggregate with GCNLayer's epilogue (csrc/gcn.hip) vs fp64, and the dropout mask of the forward, of the
    backward and of the batched-GEMM path (same counter-based mask over the flat [B, G, D] index)."""
    from nnr_amd import ops
    d = dev()
    f32 = dict(device=d, dtype=torch.float32)
    A = (torch.rand(B, G, G, generator=torch.Generator().manual_seed(1)) < 0.3).float() * torch.rand(B, G, G, generator=torch.Generator().manual_seed(2))
    z, x, bias = rnd(B, G, D, seed=3), rnd(B, G, D, seed=4), rnd(D, seed=5)
    Ad, zd, xd, bd = A.to(d), z.to(d), x.to(d), bias.to(d)
    pre = torch.relu(torch.bmm(A.double(), z.double()) + bias.double())
    # p = 0: plain epilogue
    r, y = torch.empty((B, G, D), **f32), torch.empty((B, G, D), **f32)
    ops.gcn_aggregate_fwd(Ad, zd, bd, xd, r, y, B, G, D, True, 0.0, 7)
    close(r, pre, what='gcn r')
    close(y, pre + x.double(), what='gcn y')
    y2 = torch.empty((B, G, D), **f32)
    ops.gcn_aggregate_fwd(Ad, zd, None, None, None, y2, B, G, D, False, 0.0, 7)
    close(y2, torch.bmm(A.double(), z.double()), what='gcn plain')
    # p = 0.3: same mask as the batched GEMM epilogue and as the backward
    p, seed = 0.3, 12345
    ops.gcn_aggregate_fwd(Ad, zd, bd, xd, r, y, B, G, D, True, p, seed)
    yg, rg = torch.empty((B, G, D), **f32), torch.empty((B, G, D), **f32)
    ops.gemm(Ad, zd, yg, M=G, N=D, K=G, lda=G, ldb=D, ldc=D, trans_b=True, bias=bd, act=ops.ACT_RELU, aux_out=rg, ldaux=D, resid=xd, ldres=D,
             drop=(3, p, seed, D), batch=B, strideA=G * G, strideB=G * D, strideC=G * D, stride_aux=G * D, stride_res=G * D, tile=2)
    assert torch.equal(y == 0, yg == 0)
    close(y, yg.double(), what='gcn y vs batched GEMM')
    keep = (y != 0).cpu()
    assert 0.6 < float(keep.float().mean()) < 0.8
    close(y.cpu()[keep], ((pre + x.double()) / (1 - p))[keep], what='gcn y kept')
    # backward
    dy = rnd(B, G, D, seed=6)
    dyd = dy.to(d)
    ds, dx0, dz = torch.empty((B, G, D), **f32), torch.empty((B, G, D), **f32), torch.empty((B, G, D), **f32)
    ops.gcn_aggregate_bwd(Ad, dyd, r, ds, dx0, dz, B, G, D, p, seed)
    m = keep.double() / (1 - p)
    close(dx0, dy.double() * m, what='gcn dx0')
    ds_ref = dy.double() * m * (pre > 0)
    close(ds, ds_ref, what='gcn ds')
    close(dz, torch.bmm(A.double().transpose(1, 2), ds_ref), what='gcn dz')
    ds1, dx1 = torch.empty((B, G, D), **f32), torch.empty((B, G, D), **f32)
    ops.relu_drop_bwd(dyd, r, ds1, dx1, p, seed)
    assert torch.equal(ds1, ds) and torch.equal(dx1, dx0)
    dz2 = torch.empty((B, G, D), **f32)
    ops.gcn_aggregate_bwd(Ad, dyd, None, None, None, dz2, B, G, D, 0.0, 0)
    close(dz2, torch.bmm(A.double().transpose(1, 2), dy.double()), what='gcn plain A^T')


@pytest.mark.parametrize('n,Lx,D', [(333, 32, 400), (45, 128, 400), (7, 5, 8), (50, 40, 1000)])
def test_packed_seq_sum_matches_index_add(n, Lx, D):
    """out[s] = sum over the packed rows of sequence s (the per-sequence reduction of the gate gradient, newsEncoders.py:128-129 backward)."""
    from nnr_amd import ops
    lens = _lengths(n, Lx, 31)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    plan = ops.SeqPlan(mask.clone().to(dev()), None)
    tot = int(plan.off[-1])
    x = rnd(plan.cap, D, seed=8).to(dev())
    out = torch.empty((n, D), device=dev(), dtype=torch.float32)
    ops.packed_seq_sum(x, D, plan, out)
    ref = torch.zeros((n, D), dtype=torch.float64)
    ref.index_add_(0, plan.row_seq[:tot].cpu().long(), x[:tot].cpu().double())
    close(out, ref, tol=1e-5, what='packed_seq_sum')


@pytest.mark.parametrize('dot', [False, True])
def test_pool_packed_forward_backward(dot):
    from nnr_amd import ops
    d = dev()
    n, Lx, D = 50, 128, 400
    lens = _lengths(n, Lx, 3)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    plan = ops.SeqPlan(mask.clone().to(d), None)
    off, rank = plan.off.cpu().long(), plan.rank.cpu().long()
    rows = off[:Lx][None, :] + rank[:, None]
    cap = plan.cap
    x = rnd(n, Lx, D, seed=1)
    xp = torch.zeros(cap, D)
    xp[rows[mask]] = x[mask]
    v = rnd(n, D, seed=2, scale=0.2)
    sc = rnd(n, Lx, seed=3)
    add_in = rnd(n, D, seed=4)
    scale = 0.37
    xr = x.double().requires_grad_(True)
    vr = v.double().requires_grad_(True)
    scr = sc.double().requires_grad_(True)
    score = scale * torch.einsum('nld,nd->nl', xr, vr) if dot else scr
    out_ref, a_ref = _softmax_pool_ref(xr, score, mask)
    dout = rnd(n, D, seed=5)
    dout2 = rnd(n, D, seed=6)
    (out_ref * (dout + dout2).double()).sum().backward()
    f32 = dict(device=d, dtype=torch.float32)
    xd = xp.to(d)
    alpha = torch.zeros(cap, **f32)
    out = torch.empty(n, D, **f32)
    kw = dict(x=xd, ldx=D, D=D, n=n, Lx=Lx, plan=plan, alpha=alpha)
    if dot:
        kw.update(v=v.to(d), ldv=D, scale=scale)
    else:
        scp = torch.zeros(cap)
        scp[rows[mask]] = sc[mask]
        kw.update(score=scp.to(d))
    ops.pool_fwd(out=out, ldo=D, add_in=add_in.to(d), ldadd=D, **kw)
    close(out, out_ref + add_in.double(), what='pool out')
    dx = torch.full((cap, D), 0.5, **f32)
    dscore = torch.zeros(cap, **f32)
    dv = torch.empty(n, D, **f32)
    kw.pop('score', None)
    ops.pool_bwd(dout=dout.to(d), lddo=D, dout2=dout2.to(d), lddo2=D, dx=dx, lddx=D, dx_accumulate=True, dscore=dscore,
                 dv=dv if dot else None, lddv=D, **kw)
    got = torch.zeros(n, Lx, D, dtype=torch.float64)
    got[mask] = dx.cpu().double()[rows[mask]] - 0.5
    close(got, xr.grad, what='pool dx')
    if dot:
        close(dv, vr.grad, what='pool dv')
    else:
        gs = torch.zeros(n, Lx, dtype=torch.float64)
        gs[mask] = dscore.cpu().double()[rows[mask]]
        close(gs, scr.grad, what='pool dscore')


def test_pool_backward_of_two_pools_in_one_write():
    """CNE pools every token stream twice (additive self attention, layers.py:167-175; candidate cross attention, layers.py:196-203;
    newsEncoders.py:132-137).  Round 5: the cross pool's backward runs with dx = NULL (it leaves d score and dv), the self pool's backward
    then writes  dx = alpha_s (dout + dout2) + alpha_c dout_b + scale dscore_c v  in ONE store.  Checked against fp64 autograd of the sum of
    both pools, and against the two-pass form (store, then read-modify-write) of rounds 1-4."""
    from nnr_amd import ops
    d = dev()
    n, Lx, D = 37, 128, 400
    lens = _lengths(n, Lx, 5)
    mask = torch.arange(Lx)[None, :] < lens[:, None]
    plan = ops.SeqPlan(mask.clone().to(d), None)
    off, rank = plan.off.cpu().long(), plan.rank.cpu().long()
    rows = off[:Lx][None, :] + rank[:, None]
    cap = plan.cap
    x = rnd(n, Lx, D, seed=1)
    xp = torch.zeros(cap, D)
    xp[rows[mask]] = x[mask]
    v = rnd(n, D, seed=2, scale=0.2)
    sc = rnd(n, Lx, seed=3)
    scale = 0.31
    xr, vr, scr = x.double().requires_grad_(True), v.double().requires_grad_(True), sc.double().requires_grad_(True)
    out_s, _ = _softmax_pool_ref(xr, scr, mask)
    out_c, _ = _softmax_pool_ref(xr, scale * torch.einsum('nld,nd->nl', xr, vr), mask)
    dout, dout2 = rnd(n, D, seed=5), rnd(n, D, seed=6)
    (out_s * (dout + dout2).double() + out_c * dout.double()).sum().backward()
    f32 = dict(device=d, dtype=torch.float32)
    xd, vd = xp.to(d), v.to(d)
    scp = torch.zeros(cap)
    scp[rows[mask]] = sc[mask]
    alpha_s, alpha_c = torch.zeros(cap, **f32), torch.zeros(cap, **f32)
    out = torch.empty(n, D, **f32)
    base = dict(x=xd, ldx=D, D=D, n=n, Lx=Lx, plan=plan)
    ops.pool_fwd(out=out, ldo=D, score=scp.to(d), alpha=alpha_s, **base)
    ops.pool_fwd(out=out, ldo=D, v=vd, ldv=D, scale=scale, alpha=alpha_c, **base)
    dd, dd2 = dout.to(d), dout2.to(d)
    # two passes (rounds 1-4)
    dx2 = torch.empty(cap, D, **f32)
    dv2 = torch.empty(n, D, **f32)
    ds2 = torch.zeros(cap, **f32)
    ops.pool_bwd(alpha=alpha_c, v=vd, ldv=D, scale=scale, dout=dd, lddo=D, dx=dx2, lddx=D, dv=dv2, lddv=D, **base)
    ops.pool_bwd(alpha=alpha_s, dout=dd, lddo=D, dout2=dd2, lddo2=D, dx=dx2, lddx=D, dx_accumulate=True, dscore=ds2, **base)
    # one write (round 5)
    dx1 = torch.full((cap, D), 7.0, **f32)
    dv1 = torch.empty(n, D, **f32)
    ds_c = torch.zeros(cap, **f32)
    ds1 = torch.zeros(cap, **f32)
    ops.pool_bwd(alpha=alpha_c, v=vd, ldv=D, scale=scale, dout=dd, lddo=D, dscore=ds_c, dv=dv1, lddv=D, **base)
    ops.pool_bwd(alpha=alpha_s, dout=dd, lddo=D, dout2=dd2, lddo2=D, dx=dx1, lddx=D, dscore=ds1,
                 alpha_b=alpha_c, dout_b=dd, lddo_b=D, dscore_b=ds_c, v_b=vd, ldv_b=D, scale_b=scale, **base)
    got = torch.zeros(n, Lx, D, dtype=torch.float64)
    got[mask] = dx1.cpu().double()[rows[mask]]
    close(got, xr.grad, what='two pools, one write: dx')
    close(dv1, vr.grad, what='two pools: dv')
    gs = torch.zeros(n, Lx, dtype=torch.float64)
    gs[mask] = ds1.cpu().double()[rows[mask]]
    close(gs, scr.grad, what='two pools: dscore (self)')
    live = rows[mask]
    assert torch.equal(dv1, dv2) and torch.equal(ds1, ds2)
    assert float((dx1[live.to(d)] - dx2[live.to(d)]).abs().max()) <= 1e-6 * float(dx2.abs().max())      # same terms, possibly another fma contraction
    with pytest.raises(Exception):          # incomplete second-pool arguments are refused
        ops.pool_bwd(alpha=alpha_s, dout=dd, lddo=D, dx=dx1, lddx=D, alpha_b=alpha_c, **base)


def test_pool_dense_masked_dot():
    from nnr_amd import ops
    d = dev()
    Bn, N, Cn, D = 6, 5, 19, 900
    n = Bn * N
    x = rnd(n, Cn, D, seed=1)
    v = rnd(n, D, seed=2, scale=0.1)
    cmask = torch.rand(Bn, Cn, generator=torch.Generator().manual_seed(3)) < 0.4
    cmask[:, -1] = True
    m_full = cmask[:, None, :].expand(Bn, N, Cn).reshape(n, Cn)
    scale = 1 / 15.0
    xr, vr = x.double().requires_grad_(True), v.double().requires_grad_(True)
    out_ref, _ = _softmax_pool_ref(xr, scale * torch.einsum('nld,nd->nl', xr, vr), m_full)
    dout = rnd(n, D, seed=4)
    (out_ref * dout.double()).sum().backward()
    f32 = dict(device=d, dtype=torch.float32)
    alpha = torch.empty(n * Cn, **f32)
    out = torch.empty(n, D, **f32)
    kw = dict(x=x.to(d), ldx=D, D=D, n=n, Lx=Cn, mask=cmask.to(d), mask_div=N, v=v.to(d), ldv=D, scale=scale, alpha=alpha)
    ops.pool_fwd(out=out, ldo=D, **kw)
    close(out, out_ref, what='dense pool out')
    dx = torch.empty(n * Cn, D, **f32)
    dv = torch.empty(n, D, **f32)
    ops.pool_bwd(dout=dout.to(d), lddo=D, dx=dx, lddx=D, dv=dv, lddv=D, **kw)
    close(dx.view(n, Cn, D), xr.grad, what='dense pool dx')
    close(dv, vr.grad, what='dense pool dv')


# ------------------------------------------------------------------------------------------------ SUE intra-cluster, misc
def _sue_intra_case(Bn, N, Hn, Cn, A, D, cidx):
    """sue_intra_fwd / _bwd (outputs prefilled with NaN) against explicit float64 per-cluster loops = torch_scatter's definition; -> (alpha, feat,
    dg, dkf, dqc) of the kernels."""
    from nnr_amd import ops
    d = dev()
    kf, qc, g = rnd(Bn, Hn, A, seed=1, scale=0.3), rnd(Bn, N, A, seed=2), rnd(Bn, Hn, D, seed=3)
    kr, qr, gr = (t.double().requires_grad_(True) for t in (kf, qc, g))
    s = torch.einsum('bja,bna->bnj', kr, qr) / math.sqrt(A)
    feat_ref = torch.zeros(Bn, N, Cn, D, dtype=torch.float64)
    alpha_ref = torch.zeros(Bn, N, Hn, dtype=torch.float64)
    for b in range(Bn):
        for c in range(Cn):
            sel = (cidx[b] == c).nonzero().flatten()
            if sel.numel():
                a = torch.softmax(s[b][:, sel], dim=1)
                alpha_ref[b][:, sel] = a
                feat_ref[b, :, c] = a @ gr[b, sel]
    dfeat = rnd(Bn, N, Cn, D, seed=5)
    (feat_ref * dfeat.double()).sum().backward()
    nan = lambda *shape: torch.full(shape, float('nan'), device=d, dtype=torch.float32)
    alpha, feat = nan(Bn, N, Hn), nan(Bn * N * Cn, D)
    kd, qd, gd, cd = kf.to(d), qc.to(d), g.to(d), cidx.to(d)
    ops.sue_intra_fwd(kd, qd, gd, cd, Bn, N, Hn, Cn, A, D, alpha, feat)
    close(alpha, alpha_ref, what='intra alpha')
    close(feat.view(Bn, N, Cn, D), feat_ref, what='intra feat')
    dg, dk, dq = nan(Bn, Hn, D), nan(Bn * Hn, A), nan(Bn * N, A)
    ops.sue_intra_bwd(kd, qd, gd, cd, alpha, dfeat.to(d).view(-1, D), Bn, N, Hn, Cn, A, D, dg, dk, dq)
    close(dg, gr.grad, what='intra dg')
    close(dk.view(Bn, Hn, A), kr.grad, what='intra dkf')
    close(dq.view(Bn, N, A), qr.grad, what='intra dqc')
    return alpha, feat.view(Bn, N, Cn, D), dg, dk, dq


@pytest.mark.parametrize('Bn,N,Hn,Cn,A,D', [(7, 5, 50, 19, 225, 900), (3, 2, 17, 2, 64, 52), (2, 8, 64, 32, 128, 50), (2, 1, 5, 7, 32, 260),
                                            (66, 5, 50, 18, 128, 900)])
def test_sue_intra_cluster_matches_scatter_semantics(Bn, N, Hn, Cn, A, D):
    """Cluster attention of SUE (csrc/sue_cluster.hip sue_intra_*): the default shape, fewer clusters than the backward's cluster split, the
    kernels' maxima (64 items, 32 clusters, 8 candidates, D not a multiple of 4), one candidate, and the headline launch shape."""
    cidx = torch.randint(0, Cn, (Bn, Hn), generator=torch.Generator().manual_seed(4))
    cidx[0] = Cn - 1
    _sue_intra_case(Bn, N, Hn, Cn, A, D, cidx)


@pytest.mark.parametrize('shape,pattern', [((3, 2, 6, 4, 8, 7), 'one_cluster'), ((3, 2, 6, 4, 8, 7), 'empty_ends'), ((2, 3, 5, 8, 16, 12), 'one_per_cluster'),
                                           ((9, 5, 50, 19, 32, 300), 'last_user')], ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_sue_intra_cluster_at_the_gemv_forms_edge_cases(shape, pattern):
    """The keys form at the cluster patterns the GEMV form is held to (tests/test_hip_sue_ablation_gpu.py): every item in one cluster, empty first
    and last clusters, one item per cluster (Hn <= C), a user whose items all sit in the last cluster.  Every output element is written, an
    empty cluster's feature rows are exactly zero, and two runs give the same bits."""
    from test_hip_sue_ablation_gpu import _clusters
    Bn, N, Hn, Cn, A, D = shape
    cidx = _clusters(Bn, Hn, Cn, pattern, torch.Generator().manual_seed(sum(shape) + len(pattern)))
    first, second = _sue_intra_case(*shape, cidx), _sue_intra_case(*shape, cidx)
    for a, b in zip(first, second):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    empty = (torch.nn.functional.one_hot(cidx, Cn).sum(dim=1) == 0).unsqueeze(1).expand(-1, N, -1)       # [B, N, C]
    assert bool(empty.any())                                                                             # (in each of the four cases)
    assert float(first[1].cpu()[empty].abs().sum()) == 0.0


def test_elementwise_and_optimizer():
    from nnr_amd import ops
    d = dev()
    f32 = dict(device=d, dtype=torch.float32)
    # loss / logits
    Bn, N, D = 9, 5, 900
    user, cand = rnd(Bn, N, D, seed=1, scale=0.1), rnd(Bn, N, D, seed=2, scale=0.3)
    ur, cr = user.double().requires_grad_(True), cand.double().requires_grad_(True)
    lg = (ur * cr).sum(2)
    loss_ref = -(torch.log_softmax(lg, 1)[:, 0]).mean()
    loss_ref.backward()
    logits, loss, dl = torch.empty(Bn, N, **f32), torch.empty((), **f32), torch.empty(Bn, N, **f32)
    ud, cd = user.to(d), cand.to(d)
    ops.logits_fwd(ud, cd, Bn, N, D, logits)
    ops.nls_loss(logits, Bn, N, loss, dl)
    close(logits, lg, what='logits')
    close(loss, loss_ref, tol=2e-6, what='loss')
    du, dc = torch.empty_like(ud), torch.empty_like(cd)
    ops.logits_bwd(dl, ud, cd, Bn, N, D, du, dc)
    close(du, ur.grad, what='duser')
    close(dc, cr.grad, what='dcand')
    # clip + Adam vs torch.optim.Adam on a flat buffer, 3 steps
    P = 100003
    p0, gs = rnd(P, seed=3), [rnd(P, seed=10 + i, scale=0.05 * (i + 1)) for i in range(3)]
    pr = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([pr], lr=1e-3)
    p, m, v, ss = p0.to(d).clone(), torch.zeros(P, **f32), torch.zeros(P, **f32), torch.zeros(1, **f32)
    for i, g in enumerate(gs):
        pr.grad = (g.double() / 2).clone()               # grads averaged over world_size=2
        torch.nn.utils.clip_grad_norm_([pr], 4.0)
        opt.step()
        ss.zero_()
        ops.sumsq(g.to(d), ss)
        ops.clip_adam(p, g.to(d), m, v, ss, 0.5, 4.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, i + 1)
    close(p, pr.data, tol=2e-6, what='clip+Adam')
    # colsum / small embedding / gate backward
    x = rnd(1000, 400, seed=20)
    out = torch.zeros(400, **f32)
    dyn = torch.tensor([777], dtype=torch.int32, device=d)
    ops.bias_grad(x.to(d), out, dyn=dyn)
    close(out, x[:777].double().sum(0), what='colsum')
    table = rnd(18, 50, seed=21)
    idx = torch.randint(0, 18, (320,), generator=torch.Generator().manual_seed(22)).int()
    rep = torch.zeros(320, 900, **f32)
    ops.small_embed_fwd(table.to(d), idx.to(d), rep[:, 800:], 900, 0.0, 1)
    close(rep[:, 800:850], table[idx.long()], what='small embed')
    dt = torch.zeros(18, 50, **f32)
    drep = rnd(320, 900, seed=23)
    ops.small_embed_bwd(idx.to(d), 50, drep.to(d)[:, 800:], 900, dt, 0.0, 1)
    ref = torch.zeros(18, 50, dtype=torch.float64).index_add_(0, idx.long(), drep[:, 800:850].double())
    close(dt, ref, what='small embed bwd')
    # history-shaped ids (every history ends in a run of padded slots = id 0), dropout on, every row-per-wave setting of the
    # run-merging kernel, a ragged last wave; the mask is the forward's (keep = f(seed, row * dim + c))
    for n in (3203, 17001, 50):
        g = torch.Generator().manual_seed(n)
        idx = torch.randint(0, 270, (n,), generator=g).int()
        for u0 in range(0, n, 50):
            idx[u0 + int(torch.randint(5, 50, (1,), generator=g)):u0 + 50] = 0
        drep = rnd(n, 100, seed=n + 1)
        mask = torch.zeros(n, 64, **f32)
        ops.small_embed_fwd(torch.ones(270, 50, **f32), idx.to(d), mask, 64, 0.3, 77)
        dt = torch.zeros(270, 50, **f32)
        ops.small_embed_bwd(idx.to(d), 50, drep.to(d)[:, 40:], 100, dt, 0.3, 77)
        ref = torch.zeros(270, 50, dtype=torch.float64).index_add_(0, idx.long(), drep[:, 40:90].double() * mask[:, :50].cpu().double())
        close(dt, ref, what='small embed bwd, runs, n=%d' % n)


@pytest.mark.parametrize('n', [1, 3, 1027, 1_048_579, 5_000_001, 25_600_003])
def test_sumsq_is_accurate_and_deterministic(n):
    """Global squared gradient norm (clip_grad_norm_, trainer.py:118): tail-only sizes, one unrolled trip + tail, and the CNE+SUE
    buffer's size; the same bits on every call (the ranks of a data-parallel job must agree on the clip coefficient)."""
    from nnr_amd import ops
    d = dev()
    g = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.1).to(d)
    out = torch.full((2,), 7.0, device=d, dtype=torch.float32)
    ops.sumsq(g, out[:1])
    ops.sumsq(g, out[1:])
    ref = float((g.double() ** 2).sum())
    assert abs(float(out[0]) - ref) <= 1e-5 * ref + 1e-12, (float(out[0]), ref)
    assert torch.equal(out[0], out[1])


def test_mhsa_core_over_packed_rows_equals_dense():
    """Round 5 (newsEncoders.py:187-200 over the valid token rows only): nnr_mask_cover -> nnr_seq_plan -> nnr_seq_rowmap name the rows
    that can reach the result -- every position up to a title's last valid one, ALL positions of a fully masked title --, and
    nnr_mhsa_fwd_packed / _bwd_packed find them through the row map.  Against the dense kernels on the same values (padding rows of the
    dense input filled with junk: masked keys and zero upstream gradients must make them irrelevant), prefix masks, a fully masked
    title, a title with an interior masked position, with and without the fused dropout."""
    from nnr_amd import ops
    d = dev()
    n, Lq, heads, dh = 96, 32, 20, 20
    HD = heads * dh
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, Lq + 1, (n,), generator=g)
    mask = torch.arange(Lq)[None, :] < lens[:, None]
    mask[5] = False                                   # fully masked: uniform softmax, all 32 positions are rows
    mask[9, 3] = False                                # an interior masked position (lens[9] >= 5 below): a row that exists but is masked
    mask[9, :6] = True
    mask[9, 3] = False
    md = mask.to(d)
    cover = ops.mask_cover(md)
    want_cover = mask.clone()
    want_cover[5] = True
    want_cover[9, 3] = True
    assert torch.equal(cover.cpu().bool(), want_cover)
    plan = ops.SeqPlan(cover, None)
    rowmap = ops.seq_rowmap(plan)
    rm = rowmap.cpu().view(n, Lq)
    live = rm >= 0
    assert torch.equal(live, want_cover) and int(plan.total.item()) == int(want_cover.sum())
    assert sorted(rm[live].tolist()) == list(range(int(want_cover.sum())))          # a bijection onto the packed rows
    qkv = rnd(n * Lq, 3 * HD, seed=4, scale=0.5)
    qkv[~live.reshape(-1)] = 77.0                     # junk in the dense rows that do not exist in the packed form
    dout = rnd(n * Lq, HD, seed=5)
    dout[~live.reshape(-1)] = 0.0                     # (the pooled weight of a padded position is exactly 0: no gradient arrives there)
    cap = plan.cap
    qp = torch.full((cap, 3 * HD), float('nan'))
    dp = torch.full((cap, HD), float('nan'))
    qp[rm[live]] = qkv[live.reshape(-1)]
    dp[rm[live]] = dout[live.reshape(-1)]
    qd, qpd, dd, dpd = qkv.to(d), qp.to(d), dout.to(d), dp.to(d)
    for p, seed in ((0.0, 0), (0.2, 1234)):
        out = torch.empty(n * Lq, HD, device=d)
        ops.mhsa_fwd(qd, md, n, Lq, heads, dh, out, None, 0.0, 0)
        outp = torch.full((cap, HD), float('nan'), device=d)
        ops.mhsa_fwd_packed(qpd, md, rowmap, plan, heads, dh, outp, p, seed)
        got = outp.cpu()[rm[live]]
        want = out.cpu()[live.reshape(-1)]
        if p > 0:                                     # the fused dropout is keyed by (packed row, column)
            keep = (ops.dropout(torch.ones(cap * HD, device=d), p, seed) > 0).view(cap, HD).cpu()[rm[live]]
            want = want * keep / (1 - p)
        assert bool(torch.isfinite(got).all())
        assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max())), 'packed forward (p = %g)' % p
        assert bool(torch.isnan(outp.cpu()[int(plan.total.item()):]).all())          # rows beyond the live count are never written
        dq = torch.empty(n * Lq, 3 * HD, device=d)
        if p > 0:
            dk = torch.zeros(n * Lq, HD)
            dk[live.reshape(-1)] = dout[live.reshape(-1)] * keep / (1 - p)
            ops.mhsa_bwd(qd, md, None, dk.to(d), n, Lq, heads, dh, dq, 0.0, 0)
        else:
            ops.mhsa_bwd(qd, md, None, dd, n, Lq, heads, dh, dq, 0.0, 0)
        dqp = torch.full((cap, 3 * HD), float('nan'), device=d)
        ops.mhsa_bwd_packed(qpd, md, rowmap, plan, dpd, heads, dh, dqp, p, seed)
        gotb = dqp.cpu()[rm[live]]
        wantb = dq.cpu()[live.reshape(-1)]
        assert bool(torch.isfinite(gotb).all())
        assert float((gotb - wantb).abs().max()) <= 2e-6 * max(1.0, float(wantb.abs().max())), 'packed backward (p = %g)' % p
        # round 6: GROUPED short titles (two titles of <= 16 / four of <= 8 positions per 32 x 32 problem, -inf scores between them): same rows, same values up to the
        # order of fp32 additions inside a softmax row; junk-free (NaN rows beyond the live count untouched)
        if Lq == 32:
            pair = ops.mhsa_pair_map(plan, md)
            vrow, vmask = pair[0].cpu(), pair[1].cpu()
            n16, n8 = int(plan.bs.cpu()[16]), int(plan.bs.cpu()[8])
            nvirt = n16 + (n8 - n16 + 1) // 2 + (n - n8 + 3) // 4
            assert n16 < n8 < n, 'the test batch must hold titles of 9..16 and of <= 8 positions'
            lr = vrow[:nvirt][vrow[:nvirt] >= 0]
            assert sorted(lr.tolist()) == list(range(int(plan.total.item()))) and bool((vrow[nvirt:] == -1).all())      # every packed row exactly once
            outq = torch.full((cap, HD), float('nan'), device=d)
            ops.mhsa_fwd_paired(qpd, pair, plan, heads, dh, outq, p, seed)
            gotq = outq.cpu()[rm[live]]
            assert bool(torch.isfinite(gotq).all()) and bool(torch.isnan(outq.cpu()[int(plan.total.item()):]).all())
            assert float((gotq - got).abs().max()) <= 1e-6 * max(1.0, float(got.abs().max())), 'paired forward (p = %g)' % p
            dqq = torch.full((cap, 3 * HD), float('nan'), device=d)
            ops.mhsa_bwd_paired(qpd, pair, plan, dpd, heads, dh, dqq, p, seed)
            gotqb = dqq.cpu()[rm[live]]
            assert bool(torch.isfinite(gotqb).all()) and bool(torch.isnan(dqq.cpu()[int(plan.total.item()):]).all())
            assert float((gotqb - gotb).abs().max()) <= 2e-6 * max(1.0, float(gotb.abs().max())), 'paired backward (p = %g)' % p
    with pytest.raises(Exception):                    # the packed form is the 4-head cooperative path only
        ops.mhsa_fwd_packed(qpd, md, rowmap, plan, 5, 20, outp)


def test_sumsq_over_spans_chained_on_two_streams():
    """Round 5: the gradient norm in spans (nnr_sumsq_part): the word-embedding table's span on a helper stream with its own scratch slot
    WHILE another span is summed on the main stream, the partial sums chained in a fixed order -- accurate, and the same bits every time."""
    from nnr_amd import ops
    d = dev()
    n = 25_624_708
    a, b = 18_000_000, 25_624_708
    g = (torch.randn(n, generator=torch.Generator().manual_seed(5)) * 0.1).to(d)
    side = torch.cuda.Stream()
    outs = []
    for _ in range(3):
        part = torch.full((1,), 3.0, device=d)
        mid = torch.full((1,), 5.0, device=d)
        tot = torch.full((1,), 7.0, device=d)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.sumsq_part(g[:a], part, None, slot=1)              # "table" span, helper stream, scratch slot 1
        ops.sumsq_part(g[a:a + 4], mid, None, slot=0)              # (a tiny span at the same time on the main stream, slot 0)
        torch.cuda.current_stream().wait_stream(side)
        ops.sumsq_part(g[a:b], tot, part, slot=0)                  # rest + table share
        outs.append((part.clone(), tot.clone()))
    ref_a = float((g[:a].double() ** 2).sum())
    ref = float((g.double() ** 2).sum())
    assert abs(float(outs[0][0]) - ref_a) <= 1e-5 * ref_a and abs(float(outs[0][1]) - ref) <= 1e-5 * ref
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
    one = torch.empty(1, device=d)
    ops.sumsq(g, one)
    assert abs(float(one) - float(outs[0][1])) <= 2e-6 * ref       # (another partition of the same sum: equal to rounding, not bit-equal)
    with pytest.raises(Exception):
        ops.sumsq_part(g[1:9], one, None, slot=0)                  # spans start 16-byte aligned
    with pytest.raises(Exception):
        ops.sumsq_part(g[:8], one, None, slot=9)


def test_slot_spread_column_sums():
    """Long reductions into a short vector (bias gradients, dw2 of the additive attention) go through the per-stream slot
    workspace (nnr_slot_workspace_floats): same sums as the direct form; the second call, on the same stream and on a side stream
    with its own workspace, must be exact too."""
    from nnr_amd import ops
    d = dev()
    f32 = dict(device=d, dtype=torch.float32)
    x = rnd(20000, 400, seed=31)
    dyn = torch.tensor([19001], dtype=torch.int32, device=d)
    out = torch.zeros(400, **f32)
    xd = x.to(d)
    ops.bias_grad(xd, out, dyn=dyn)
    ref = x[:19001].double().sum(0)
    close(out, ref, what='colsum (slots)')
    ops.bias_grad(xd, out, dyn=dyn)
    close(out, 2 * ref, what='colsum (slots), second call')
    th = torch.tanh(rnd(20000, 200, seed=32))
    ds = rnd(20000, 1, seed=33).reshape(-1)
    w2 = rnd(1, 200, seed=34)
    dw2 = torch.zeros(1, 200, **f32)
    ref_dw2 = (ds.double()[:, None] * th.double()).sum(0)
    ref_dpre = ds.double()[:, None] * w2.double() * (1 - th.double() ** 2)
    side = torch.cuda.Stream()
    for k, stream in enumerate((torch.cuda.current_stream(), torch.cuda.current_stream(), side)):
        t = th.to(d)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops.tanh_score_bwd(t, ds.to(d), w2.to(d), dw2, None, 200)
        torch.cuda.current_stream().wait_stream(stream)
        close(dw2.reshape(-1), (k + 1) * ref_dw2, what='tanh score bwd dw2 (slots), call %d' % k)
        close(t, ref_dpre, what='tanh score bwd dpre')
    # round 4: every workgroup stores to its own slot row and the rows are added in a fixed order: bit-identical from run to run,
    # for small inputs too (one to a few workgroups), with a device-side row count, and on a dirty workspace (nothing relies on zeros)
    for ws in ops._SLOT_WS.values():
        ws.fill_(float('nan'))
    for rows, live in ((20000, 19001), (300, 300), (7, 5), (4000, 0)):
        dyn = torch.tensor([live], dtype=torch.int32, device=d)
        outs = []
        for rep in range(2):
            o = torch.zeros(400, **f32)
            ops.bias_grad(xd[:rows], o, dyn=dyn)
            t2 = th[:rows].to(d)
            g2 = torch.zeros(1, 200, **f32)
            plan = type('P', (), {'total': dyn, 'cap': rows})()
            ops.tanh_score_bwd(t2, ds[:rows].to(d), w2.to(d), g2, plan, 200)
            outs.append((o, g2, t2))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        close(outs[0][0], x[:live].double().sum(0), what='colsum %d of %d rows' % (live, rows))
        close(outs[0][1].reshape(-1), (ds.double()[:live, None] * th.double()[:live]).sum(0), what='dw2 %d of %d rows' % (live, rows))
        if live:
            close(outs[0][2][:live], ref_dpre[:live], what='dpre %d of %d rows' % (live, rows))


# ------------------------------------------------------------------------------------------------ MFMA attention core
@pytest.mark.parametrize('saved_prob', [True, False])
@pytest.mark.parametrize('n,Lq,heads,dh', [(7, 32, 20, 20), (5, 50, 20, 20), (3, 5, 2, 4), (2, 20, 4, 8), (3, 17, 6, 10)])
def test_mhsa_core_forward_backward(n, Lq, heads, dh, saved_prob):
    from nnr_amd import ops
    d = dev()
    HD = heads * dh
    qkv = rnd(n * Lq, 3 * HD, seed=1, scale=0.7)
    mask = torch.rand(n, Lq, generator=torch.Generator().manual_seed(2)) < 0.7
    mask[0] = False                                   # a fully masked sample: softmax must stay finite (uniform over keys)
    mask[1] = True
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, s * HD:(s + 1) * HD].reshape(n, Lq, heads, dh) for s in range(3))
    s_ = torch.einsum('nqhd,nkhd->nhqk', q, k) / math.sqrt(dh)
    s_ = torch.where(mask[:, None, None, :], s_, torch.full_like(s_, -1e9))
    ref = torch.einsum('nhqk,nkhd->nqhd', torch.softmax(s_, 3), v).reshape(n * Lq, HD)
    dout = rnd(n * Lq, HD, seed=3)
    (ref * dout.double()).sum().backward()
    out = torch.empty(n * Lq, HD, device=d)
    prob = torch.empty(ops.mhsa_prob_size(n, Lq, heads), device=d) if saved_prob else None     # None: backward recomputes P
    qd = qkv.to(d)
    ops.mhsa_fwd(qd, mask.to(d), n, Lq, heads, dh, out, prob)
    close(out, ref, what='mhsa out')
    dqkv = torch.full_like(qd, 3.0)
    ops.mhsa_bwd(qd, mask.to(d), prob, dout.to(d), n, Lq, heads, dh, dqkv)
    close(dqkv, x.grad, what='mhsa dqkv')
    # fused dropout == the standalone dropout kernel on the output / on the upstream gradient, bit for bit
    p_, seed = 0.2, 1234
    out_d = torch.empty_like(out)
    ops.mhsa_fwd(qd, mask.to(d), n, Lq, heads, dh, out_d, prob, p_, seed)
    assert torch.equal(out_d, ops.dropout(out, p_, seed)), 'fused dropout (forward)'
    dq1, dq2 = torch.empty_like(qd), torch.empty_like(qd)
    ops.mhsa_bwd(qd, mask.to(d), prob, dout.to(d), n, Lq, heads, dh, dq1, p_, seed)
    ops.mhsa_bwd(qd, mask.to(d), prob, ops.dropout(dout.to(d), p_, seed), n, Lq, heads, dh, dq2)
    assert torch.equal(dq1, dq2), 'fused dropout (backward)'


def test_embed_gather_scatter_and_transpose():
    from nnr_amd import ops
    d = dev()
    V, E, n = 500, 300, 3000
    table = rnd(V, E, seed=1)
    idx = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(2)).int()
    out = ops.embed_gather(table.to(d), idx.to(d), 0.0, 1)
    close(out, table[idx.long()], tol=0, what='gather')
    dropped = ops.embed_gather(table.to(d), idx.to(d), 0.25, 9)
    keep = dropped != 0
    assert abs(float(keep.float().mean()) - 0.75) < 0.01
    g = rnd(n, E, seed=3)
    dt = torch.zeros(V, E, device=d)
    ops.embed_scatter(g.to(d), idx.to(d), dt, 0.25, 9)
    ref = torch.zeros(V, E, dtype=torch.float64).index_add_(0, idx.long(), (g.double() * keep.cpu().double() / 0.75))
    close(dt, ref, what='scatter with the same mask')
    a = rnd(37, 5, seed=4)
    o = torch.empty(5, 37, device=d)
    ops.transpose2d(a.to(d), o, 37, 5)
    close(o, a.t(), tol=0, what='transpose')
    # the user vector repeated over the candidates (userEncoders.py:172,190) and its backward: the sum over the copies in ascending order
    for B, N, D in ((64, 5, 400), (3, 1, 7), (17, 64, 33)):
        u = rnd(B, D, seed=5)
        rep = ops.expand_rows(u.to(d), N)
        assert rep.shape == (B, N, D)
        close(rep, u[:, None, :].expand(B, N, D), tol=0, what='expand_rows')
        g = rnd(B, N, D, seed=6)
        want = g[:, 0].clone()
        for j in range(1, N):
            want += g[:, j]
        close(ops.expand_rows_bwd(g.to(d)), want, tol=0, what='expand_rows_bwd (ascending fp32 sum)')


@pytest.mark.parametrize('M,N,K,live', [(3000, 400, 200, 2500), (70000, 400, 200, 70000), (130, 64, 36, 130)])
def test_gemm_epilogue_gate_backward(M, N, K, live):
    """nnr_gemm_args.pre_add / gate_bwd: the GEMM that completes dHt (= pre_add + A . B^T) applies the cross-selective gate's backward
    in its epilogue -- dH = dHt * G, d pre = dHt * H * G * (1 - G) (newsEncoders.py:128-131) -- bit-for-bit what the accumulate-GEMM
    followed by nnr_gate_bwd gives."""
    from nnr_amd import ops
    d = dev()
    a, w = rnd(M, K, seed=1).to(d), rnd(N, K, seed=2).to(d)
    dht = rnd(M, N, seed=3).to(d)
    G, H = torch.sigmoid(rnd(M, N, seed=4)).to(d), rnd(M, N, seed=5).to(d)
    dyn = torch.tensor([live], dtype=torch.int32, device=d)
    plan = type('P', (), {'total': dyn, 'cap': M})()
    ref_dht = dht.clone()
    ops.gemm(a, w, ref_dht, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, accumulate=True, dyn=dyn, dyn_dim=1)
    rdH, rdpre = torch.zeros(M, N, device=d), torch.zeros(M, N, device=d)
    ops.gate_bwd(ref_dht, H, G, rdH, rdpre, plan, N)
    dH, dpre = torch.zeros(M, N, device=d), torch.zeros(M, N, device=d)
    ops.gemm(a, w, dH, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, dyn=dyn, dyn_dim=1, pre_add=dht, ldpre=N, gate_bwd=True, mul=G, ldmul=N, resid=H, ldres=N,
             aux_out=dpre, ldaux=N)
    torch.cuda.synchronize()
    assert torch.equal(dH[:live], rdH[:live]) and torch.equal(dpre[:live], rdpre[:live])
    assert float(dH[live:].abs().max()) == 0.0 if live < M else True
    x = dht.double().cpu() + a.double().cpu() @ w.double().cpu().t()
    close(dH[:live], (x * G.double().cpu())[:live], tol=2e-5, what='dH')
    close(dpre[:live], (x * H.double().cpu() * G.double().cpu() * (1 - G.double().cpu()))[:live], tol=2e-5, what='d pre')


def test_gemm_fused_bias_gradient():
    """colsum_out of the weight-gradient GEMM == column sums of dy over the live rows (split-K, dynamic K)."""
    from nnr_amd import ops
    d = dev()
    R, used, N, K = 6000, 4711, 200, 400
    dy, x = rnd(R, N, seed=1), rnd(R, K, seed=2)
    dw = torch.zeros(N, K, device=d)
    db = torch.full((N,), 0.25, device=d)
    dyn = torch.tensor([used], dtype=torch.int32, device=d)
    ops.linear_bwd_weight(dy.to(d), x.to(d), dw, dyn=dyn, db=db)
    close(dw, dy[:used].double().t() @ x[:used].double(), tol=5e-5, what='dw')
    close(db, 0.25 + dy[:used].double().sum(0), tol=5e-5, what='fused db')


@pytest.mark.parametrize('V,E,cap,live,p', [(500, 300, 3000, 3000, 0.0), (60000, 300, 20000, 15111, 0.2), (37, 300, 4100, 4000, 0.2), (900, 64, 1000, 7, 0.5),
                                             (5000, 320, 9000, 9000, 0.1), (50, 300, 640, 0, 0.2)])
def test_sorted_segmented_embedding_gradient_is_exact_and_reproducible(V, E, cap, live, p):
    """csrc/sort.hip: token rows sorted by word id (stable radix sort, pad key for rows beyond the live count) + segmented reduction
    = the f32-atomic scatter's result (same dropout mask) = the fp64 reference, and BIT-IDENTICAL from run to run; ids are heavily
    skewed (one word owns a third of the rows: a segment of hundreds of 32-row chunks), some ids invalid (negative: skipped)."""
    from nnr_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(V + cap)
    ids = torch.randint(0, V, (cap,), generator=g).int()
    hot = torch.rand(cap, generator=g)
    ids[hot < 0.33] = 3 % V                                  # one very long segment
    ids[(hot > 0.33) & (hot < 0.45)] = (V - 1)               # ... and the largest id (next to the pad key)
    ids[::97] = -1                                           # invalid ids are skipped by both forms
    dout = rnd(cap, E, seed=cap)
    total = torch.tensor([live], dtype=torch.int32, device=d)
    idd, dd = ids.to(d), dout.to(d)
    ref = torch.zeros(V, E, device=d)
    ops.embed_scatter(dd, idd, ref, p, 77, dyn=total)
    outs = []
    for rep in range(2):
        ts = ops.TokenSort(idd, total, V)
        torch.cuda.synchronize()                                 # (the sort runs on the leaf stream)
        keys = ts.keys.cpu().long()
        rows = ts.rows.cpu().long()
        valid = (torch.arange(cap) < live) & (ids >= 0)
        nv = int(valid.sum())
        assert bool((keys[:nv] < V).all()) and bool((keys[nv:] == V).all()) and bool((keys[1:] >= keys[:-1]).all())
        assert torch.equal(keys[:nv], ids.long()[rows[:nv]]) and sorted(rows.tolist()) == list(range(cap))
        if nv > 1:
            same = keys[1:nv] == keys[:nv - 1]
            assert bool((rows[1:nv][same] > rows[:nv - 1][same]).all())      # stable: ascending row order inside a word's segment
        o = torch.zeros(V, E, device=d)
        ops.embed_scatter_sorted(dd, ts, o, p, 77)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    close(outs[0], ref, tol=2e-5, what='sorted vs atomic scatter')
    keep = (ops.dropout(torch.ones(cap, E, device=d), p, 77) != 0).double().cpu() / (1.0 - p) if p > 0 else torch.ones(cap, E, dtype=torch.float64)
    want = torch.zeros(V, E, dtype=torch.float64)
    sel = (torch.arange(cap) < live) & (ids >= 0)
    want.index_add_(0, ids[sel].long(), (dout.double() * keep)[sel])
    close(outs[0], want, tol=2e-6, what='sorted vs fp64')


TN_PIPE_TILES = [20, 26, 27, 30, 32]
TN_NO_GATHER = [26]         # gen-2 loop: gathered B rows only with the 256-float pitch (tile 27)


@pytest.mark.parametrize('tile', TN_PIPE_TILES)
@pytest.mark.parametrize('M,N,K,split', [(832, 300, 5000, 4), (400, 400, 777, 1), (200, 400, 3333, 3), (1664, 300, 20000, 7), (900, 900, 4352, 2),
                                         (36, 20, 50, 2), (128, 80, 16, 1), (132, 84, 40, 3)])
def test_gemm_pipelined_tn_tiles(tile, M, N, K, split):
    """The LDS-DMA staged weight-gradient kernel (gemm_tn_pipe_kernel): ragged tile edges (zero page), reduction lengths that
    are not multiples of the stage depth, fewer stages than buffers, split-K slices that come out empty, device-side K,
    gathered B rows with negative (= zero) entries, fused column sums, accumulation into a running gradient."""
    from nnr_amd import ops
    d = dev()
    at, bt = rnd(K, M, seed=4), rnd(K, N, seed=3)
    base = rnd(M, N, seed=5)
    o = base.to(d).clone()
    ops.gemm(at.to(d), bt.to(d), o, M=M, N=N, K=K, lda=M, ldb=N, ldc=N, trans_a=True, trans_b=True, split_k=split, atomic=True, tile=tile)
    close(o, base.double() + at.double().t() @ bt.double(), tol=5e-5, what='TN pipe tile %d' % tile)
    # device-side K + gathered B rows + fused column sums, operands as column slices of wider buffers (the dW_hh shape)
    used = max(1, (K * 3) // 4)
    lda, ldb = M + 64, N + 8
    A2 = rnd(K, lda, seed=6); B2 = rnd(K, ldb, seed=7)
    bidx = torch.randint(0, K, (K,), generator=torch.Generator().manual_seed(8)).int()
    bidx[::7] = -1
    dyn = torch.tensor([used], dtype=torch.int32, device=d)
    o = torch.zeros(M, N, device=d)
    cs = torch.zeros(M, device=d)
    A2d, B2d = A2.to(d), B2.to(d)
    if tile in TN_NO_GATHER:
        bidx = torch.arange(K).int()
    ops.gemm(A2d[:, 64:], B2d[:, 8:], o, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=N, trans_a=True, trans_b=True, split_k=split, atomic=True,
             b_idx=None if tile in TN_NO_GATHER else bidx.to(d), dyn=dyn, dyn_dim=2, colsum_out=cs, tile=tile)
    a_ = A2[:used, 64:].double()
    b_ = B2[:, 8:].double()[bidx[:used].long().clamp_min(0)] * (bidx[:used] >= 0).double()[:, None]
    close(o, a_.t() @ b_, tol=5e-5, what='TN pipe gather dyn')
    close(cs, a_.sum(dim=0), tol=5e-5, what='TN pipe column sums')


@pytest.mark.parametrize('tile', [2, 6, 20, 26, 27, 30, 32])
@pytest.mark.parametrize('M,N,K,split', [(400, 400, 7000, 40), (200, 400, 333, 9), (832, 200, 5000, 13), (1664, 300, 9000, 16), (36, 20, 50, 3), (132, 84, 16, 5)])
def test_split_k_slabs_reduce_in_fixed_order(tile, M, N, K, split):
    """nnr_gemm_args.slab: every slice of a split-K weight-gradient launch stores its partial result, a second launch adds the live
    slices in slice order (csrc/gemm.hip: splitk_reduce_kernel) -- same value as the f32-atomic epilogue up to rounding order, and
    BIT-IDENTICAL from run to run (the atomic form is not), including the fused column sums, a device-side reduction length (fewer
    live slices than the host sized for, down to none) and gathered rows."""
    from nnr_amd import ops
    d = dev()
    gather = tile in (20, 27, 32) and N <= 256
    A, Bm = rnd(K, M + 64, seed=6).to(d), rnd(K, N + 8, seed=7).to(d)
    bidx = torch.randint(0, K, (K,), generator=torch.Generator().manual_seed(8)).int()
    bidx[::7] = -1
    base = rnd(M, N, seed=5).to(d)
    for used in (K, max(1, K // 3), 1, 0):
        dyn = torch.tensor([used], dtype=torch.int32, device=d)
        res = {}
        for mode in ('slab', 'slab', 'atomic'):
            ops.TN_SLAB = mode == 'slab'
            try:
                o, cs = base.clone(), torch.full((M,), 0.5, device=d)
                ops.gemm(A[:, 64:], Bm[:, 8:], o, M=M, N=N, K=K, lda=M + 64, ldb=N + 8, ldc=N, trans_a=True, trans_b=True, split_k=split, atomic=True,
                         b_idx=bidx.to(d) if gather else None, dyn=dyn, dyn_dim=2, colsum_out=cs, tile=tile)
            finally:
                ops.TN_SLAB = True
            res.setdefault(mode, []).append((o, cs))
        torch.cuda.synchronize()
        (o1, c1), (o2, c2) = res['slab']
        assert torch.equal(o1, o2) and torch.equal(c1, c2), 'slab mode is not reproducible (tile %d, used %d)' % (tile, used)
        a_ = A[:used, 64:].double().cpu()
        b_ = Bm[:, 8:].double().cpu()
        b_ = (b_[bidx[:used].long().clamp_min(0)] * (bidx[:used] >= 0).double()[:, None]) if gather else b_[:used]
        close(o1, base.double().cpu() + a_.t() @ b_, tol=5e-5, what='slab TN tile %d used %d' % (tile, used))
        close(c1, 0.5 + a_.sum(dim=0), tol=5e-5, what='slab column sums')
        close(res['atomic'][0][0], o1, tol=2e-5, what='atomic vs slab')


def test_transpose_batch_and_weight_transpose_cache():
    """nnr_transpose_batch: several transposes in one launch (ragged sizes, not multiples of the 32 x 32 tile); ops.wt / wt_prefetch:
    the cached W^T follows the parameter through optimizer steps (PARAM_EPOCH), in-place edits (version counter) and is never
    served for a different tensor that happens to reuse the pointer."""
    import ctypes as C
    from nnr_amd import _lib as L, ops
    from nnr_amd.layers import PARAM_EPOCH
    d = dev()
    shapes = [(900, 900), (225, 900), (37, 5), (1, 64), (400, 200)]
    ins = [rnd(r, c, seed=i).to(d) for i, (r, c) in enumerate(shapes)]
    outs = [torch.empty(c, r, device=d) for r, c in shapes]
    arr = (L.TransposeDesc * len(shapes))()
    for k, (a, o) in enumerate(zip(ins, outs)):
        arr[k].inp, arr[k].out, arr[k].rows, arr[k].cols = a.data_ptr(), o.data_ptr(), a.shape[0], a.shape[1]
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(d)
    L.check(L.lib().nnr_transpose_batch(C.c_void_p(tab.data_ptr()), len(shapes), ops._s()), 'nnr_transpose_batch')
    for a, o in zip(ins, outs):
        assert torch.equal(o, a.t().contiguous())
    w = torch.nn.Parameter(rnd(300, 200, seed=9).to(d))
    t1 = ops.wt(w)
    assert torch.equal(t1, w.detach().t().contiguous()) and ops.wt(w) is t1
    with torch.no_grad():
        w.mul_(2.0)                                        # in-place edit: version counter
    assert torch.equal(ops.wt(w), w.detach().t().contiguous())
    w.data.add_(1.0)                                       # raw-pointer style update (as the fused Adam kernel): only PARAM_EPOCH tells
    PARAM_EPOCH[0] += 1
    ops.wt_prefetch(d)
    torch.cuda.synchronize()
    assert torch.equal(ops.wt(w), w.detach().t().contiguous())
    w2 = torch.nn.Parameter(rnd(300, 200, seed=10).to(d))
    assert torch.equal(ops.wt(w2), w2.detach().t().contiguous())


def test_bx3_images_of_a_weight_transpose_follow_a_torch_optimizer_step(monkeypatch):
    """The bf16x3 images of a cached W^T are derived from the copy, not from the parameter.  A torch optimizer step moves the parameter's
    version counter but not PARAM_EPOCH: wt() rewrites the copy in place, and the copy's images must be re-split too, or the next dX GEMM on
    the bf16x3 path multiplies by the old weights."""
    from nnr_amd import ops
    d = dev()
    M, N, K = 4096, 256, 256
    monkeypatch.setattr(ops, 'BX3', [True])
    w = torch.nn.Parameter(rnd(N, K, seed=31, scale=0.1).to(d))
    dy = rnd(M, N, seed=32).to(d)
    seen = ops.BX3_SEEN.get((M, K, N, 'weight'), 0)
    ops.linear_bwd_data(dy, w)
    w.grad = torch.ones_like(w)
    torch.optim.SGD([w], lr=1.0, foreach=False).step()      # every weight moves by 1.0: far beyond the bf16x3 error
    out = ops.linear_bwd_data(dy, w)
    assert ops.BX3_SEEN.get((M, K, N, 'weight'), 0) == seen + 2       # both products took the bf16x3 path
    ops.BX3[0] = False
    ref = ops.linear_bwd_data(dy, w)
    close(out, ref, tol=2e-5 * max(1.0, math.sqrt(N / 100.0)), what='dX after a torch optimizer step')


