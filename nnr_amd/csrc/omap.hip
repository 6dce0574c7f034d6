// The OMAP (Hi-Fi Ark) user encoder, userEncoders.py:357-374.  Per user b with X = hist[b] [H, D], C = cand[b] [N, D], key / row mask m [H],
// W [D, K] and s = sqrt(D):
//   S = X X^T / s ; alpha = softmax_j(m[j] ? S[i,j] : -1e9) ; Y = X + alpha X                  (projection-free self-attention with a residual)
//   b = Y W / s   ; beta  = softmax_k(m[i] ? b[i,k] : -1e9) ; R = beta^T Y  [K, D]              (archives: a softmax over the HEADS; a padded row
//                                                                                                 carries 1/K and contributes Y[i] / K)
//   t = C R^T / s ; gamma = softmax_k(t) ; U = gamma R       [N, D]                              (one user vector per candidate)
// The three [H, H, D] products of each direction run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, operand / accumulator maps as in
// mhsa.hip); everything else is a pooling over K <= 16 heads.  Nothing larger than [B, H, H] / [B, H, D] is stored.
//
// Work split.  D has three full reductions per direction (S, b, t forward; d gamma, d beta, d alpha backward), everything between them is
// local to a column: kernels that reduce over D take one workgroup per user and stream D in chunks of 64 columns, kernels that do not take
// one workgroup per (user, slice of 64 columns).
//   forward 1  omap_alpha_kernel   per user: S on the MFMA from [HP, 64] chunks of X in LDS (the next chunk's loads are in registers while
//                                  the current one is multiplied), masked row softmax -> alpha.
//   forward 2  omap_mix_kernel     per (user, slice): Y = X + alpha X on the MFMA (alpha is the A operand, read once into registers), Y is SAVED
//                                  for the backward pass (same size as X; recomputing it there would repeat this whole launch), and the slice's
//                                  share of b -> workspace.
//   forward 3  omap_pool_kernel    per user: b summed over the slices in slice order, beta, R, t, gamma, U.
//   backward 1 omap_bwd_pool_kernel    per user: d gamma, dt, dR (workspace), dC, d beta, db (workspace).
//   backward 2 omap_bwd_dalpha_kernel  per user: dY = beta dR + db W^T / s chunk by chunk into LDS (never stored), d alpha = dY X^T on the MFMA,
//                                      dS (zero where the key is masked: masked_fill passes no gradient, also for a user without history
//                                      whose alpha is 1/H), G = (dS + dS^T) / s -> workspace.
//   backward 3 omap_bwd_dx_kernel      per (user, slice): dY again (K FMAs per element, cheaper than a [B, H, D] round trip), dX = dY + alpha^T dY
//                                      + G X on the MFMA, and the user's rows of dW = Y^T db / s -> workspace.
//   backward 4 partial_rows_sum_kernel dW += the per-user rows added in user order by one thread per element: no float atomics into shared
//                                      destinations, same inputs -> same bits (nnr_colsum would do the same in two launches).
// The regulariser coef * ||(W^T W) o (J - I)||_F is one workgroup forward (Off and Omega stay on the device for the backward pass) and one
// elementwise launch backward, scaled by the device-side upstream gradient; an exactly zero Omega gives an exactly zero gradient, as torch.
// Limits: H <= 96 (three 32-row MFMA blocks: the [HP, HP] score tile and a chunk share 64 KB of LDS), K <= 16.
#include <math.h>
#include "common.h"

namespace {

constexpr int OM_KC = 64;                    // columns of a streamed chunk / of a slice
constexpr int OM_LD = OM_KC + 1;             // LDS row stride of a chunk (odd: a thread per row walks it conflict-free)
constexpr int OM_MAXK = 16;
constexpr int OM_MAXH = 96;
constexpr int OM_LDS_BYTES = 64 * 1024;      // dynamic LDS a launch may ask for without an attribute

__device__ __forceinline__ int om_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }
__device__ __forceinline__ f32x16 om_zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// in-place softmax of v[0..K) (K <= 16, registers)
__device__ __forceinline__ void om_softmax_k(float (&v)[OM_MAXK], int K) {
  float m = -INFINITY, sm = 0.f;
#pragma unroll
  for (int k = 0; k < OM_MAXK; ++k)
    if (k < K) m = fmaxf(m, v[k]);
#pragma unroll
  for (int k = 0; k < OM_MAXK; ++k)
    if (k < K) { v[k] = expf(v[k] - m); sm += v[k]; }
#pragma unroll
  for (int k = 0; k < OM_MAXK; ++k)
    if (k < K) v[k] = v[k] / sm;
}

// ---------------------------------------------------------------------------------------------------------------- forward 1
template <int NB>
__global__ __launch_bounds__(256) void omap_alpha_kernel(const float* __restrict__ X, int ldf, const uint8_t* __restrict__ mask, int H, int D,
                                                         float s, float* __restrict__ alpha) {
  constexpr int HP = NB * 32, NT = (NB * NB + 3) / 4, NPRE = NB * 8, SS = HP + 1;
  extern __shared__ __align__(16) float om_smem[];
  float* sX = om_smem;                        // [HP][OM_LD], later the score tile [HP][SS]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int c = tid & 63, r0 = tid >> 6;
  const float* Xb = X + (long)b * H * ldf;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = om_zero16();
  float pre[NPRE];
#pragma unroll
  for (int u = 0; u < NPRE; ++u) {
    const int i = r0 + 4 * u;
    pre[u] = (c < D && i < H) ? Xb[(long)i * ldf + c] : 0.f;
  }
  for (int c0 = 0; c0 < D; c0 += OM_KC) {
    __syncthreads();                          // the previous chunk has been multiplied
#pragma unroll
    for (int u = 0; u < NPRE; ++u) sX[(r0 + 4 * u) * OM_LD + c] = pre[u];
    __syncthreads();
    if (c0 + OM_KC < D) {
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int i = r0 + 4 * u;
        pre[u] = (c0 + OM_KC + c < D && i < H) ? Xb[(long)i * ldf + c0 + OM_KC + c] : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int tile = w + 4 * t;
      if (tile < NB * NB) {
        const float* xa = sX + ((tile / NB) * 32 + l31) * OM_LD + half;
        const float* xb = sX + ((tile % NB) * 32 + l31) * OM_LD + half;
#pragma unroll 8
        for (int ks = 0; ks < OM_KC; ks += 2) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[ks], xb[ks], acc[t], 0, 0, 0);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = w + 4 * t;
    if (tile < NB * NB) {
      const int ib = tile / NB, jb = tile % NB;
#pragma unroll
      for (int r = 0; r < 16; ++r) sX[(ib * 32 + om_row(r, half)) * SS + jb * 32 + l31] = acc[t][r] / s;
    }
  }
  __syncthreads();
  // masked softmax over the keys, one wave per query row (every row is computed, padded ones too)
  const uint8_t* mb = mask ? mask + (long)b * H : nullptr;
  for (int i = w; i < H; i += 4) {
    float* row = sX + i * SS;
    float m = -INFINITY;
    for (int j = lane; j < H; j += 64) {
      const float v = (mb && !mb[j]) ? -1e9f : row[j];
      row[j] = v;
      m = fmaxf(m, v);
    }
    m = wave_max(m);
    float sm = 0.f;
    for (int j = lane; j < H; j += 64) {
      const float e = expf(row[j] - m);
      row[j] = e;
      sm += e;
    }
    sm = wave_sum(sm);
    for (int j = lane; j < H; j += 64) alpha[((long)b * H + i) * H + j] = row[j] / sm;
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward 2
// grid B * S.  Y[b, :, slice] = X + alpha X, bpart[b, slice, i, k] = sum over the slice's columns of Y[i, c] W[c, k]
template <int NB>
__global__ __launch_bounds__(256) void omap_mix_kernel(const float* __restrict__ X, int ldf, const float* __restrict__ alpha,
                                                       const float* __restrict__ W, int H, int D, int K, int S, float* __restrict__ Y,
                                                       float* __restrict__ bpart) {
  constexpr int HP = NB * 32, NT = (NB * 2 + 3) / 4, NA = NB * 16;
  extern __shared__ __align__(16) float om_smem[];
  float* sX = om_smem;                        // [HP][OM_LD]: X, then Y
  float* sW = sX + HP * OM_LD;                // [OM_KC][K]
  const int b = blockIdx.x / S, sl = blockIdx.x - b * S, c0 = sl * OM_KC;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, half = lane >> 5;
  {
    const int c = tid & 63;
    const bool cl = c0 + c < D;
    const float* xs = X + (long)b * H * ldf + c0 + c;
    for (int i = tid >> 6; i < HP; i += 4) sX[i * OM_LD + c] = (cl && i < H) ? xs[(long)i * ldf] : 0.f;
    for (int i = tid; i < OM_KC * K; i += 256) sW[i] = ((long)c0 * K + i < (long)D * K) ? W[(long)c0 * K + i] : 0.f;
  }
  __syncthreads();
  const float* ab = alpha + (long)b * H * H;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = om_zero16();
    const int tile = w + 4 * t;
    if (tile < NB * 2) {
      const int ib = tile >> 1, cb = tile & 1, i = ib * 32 + l31;
      float av[NA];
#pragma unroll
      for (int u = 0; u < NA; ++u) {
        const int j = 2 * u + half;
        av[u] = (i < H && j < H) ? ab[(long)i * H + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < NA; ++u) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], sX[(2 * u + half) * OM_LD + cb * 32 + l31], acc[t], 0, 0, 0);
    }
  }
  __syncthreads();                            // every product has read X: the tile becomes Y
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = w + 4 * t;
    if (tile < NB * 2) {
      const int ib = tile >> 1, cc = (tile & 1) * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ib * 32 + om_row(r, half);
        const float y = sX[i * OM_LD + cc] + acc[t][r];
        sX[i * OM_LD + cc] = y;
        if (i < H && c0 + cc < D) Y[((long)b * H + i) * D + c0 + cc] = y;
      }
    }
  }
  __syncthreads();
  for (int p = tid; p < H * K; p += 256) {
    const int i = p / K, k = p - i * K;
    const float* y = sX + i * OM_LD;
    float sum = 0.f;
#pragma unroll 8
    for (int cc = 0; cc < OM_KC; ++cc) sum += y[cc] * sW[cc * K + k];      // (columns past D hold zeros)
    bpart[((long)blockIdx.x * H) * K + p] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward 3
// grid B.  LDS: beta [H*K], t / gamma [N*K]
__global__ __launch_bounds__(256) void omap_pool_kernel(const float* __restrict__ Y, const float* __restrict__ cand, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ bpart, int N, int H, int D, int K, int S, float s,
                                                        float* __restrict__ beta, float* R, float* __restrict__ gamma,
                                                        float* __restrict__ out) {
  extern __shared__ __align__(16) float om_smem[];
  float* sBeta = om_smem;
  float* sT = sBeta + H * K;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < H; i += 256) {
    const bool live = !mask || mask[(long)b * H + i];
    float v[OM_MAXK];
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) v[k] = 0.f;
    for (int sl = 0; sl < S; ++sl) {          // slice order: fixed
      const float* bp = bpart + (((long)b * S + sl) * H + i) * K;
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) v[k] += bp[k];
    }
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) v[k] = live ? v[k] / s : -1e9f;
    om_softmax_k(v, K);
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k)
      if (k < K) {
        sBeta[i * K + k] = v[k];
        beta[((long)b * H + i) * K + k] = v[k];
      }
  }
  __syncthreads();
  // archives R[k, c] = sum_i beta[i, k] Y[i, c]: a thread per column
  const float* Yb = Y + (long)b * H * D;
  float* Rb = R + (long)b * K * D;
  for (int c = tid; c < D; c += 256) {
    float acc[OM_MAXK];
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) acc[k] = 0.f;
#pragma unroll 4
    for (int i = 0; i < H; ++i) {
      const float y = Yb[(long)i * D + c];
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) acc[k] += sBeta[i * K + k] * y;
    }
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k)
      if (k < K) Rb[(long)k * D + c] = acc[k];
  }
  __threadfence();
  __syncthreads();                            // R of this user is complete and visible to the workgroup
  const float* Cb = cand + (long)b * N * D;
  for (int p = w; p < N * K; p += 4) {
    const int n = p / K, k = p - n * K;
    float d = 0.f;
    for (int c = lane; c < D; c += 64) d += Cb[(long)n * D + c] * Rb[(long)k * D + c];
    d = wave_sum(d);
    if (lane == 0) sT[p] = d / s;
  }
  __syncthreads();
  for (int n = tid; n < N; n += 256) {
    float v[OM_MAXK];
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) v[k] = k < K ? sT[n * K + (k < K ? k : 0)] : 0.f;
    om_softmax_k(v, K);
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k)
      if (k < K) {
        sT[n * K + k] = v[k];
        gamma[((long)b * N + n) * K + k] = v[k];
      }
  }
  __syncthreads();
  for (int c = tid; c < D; c += 256) {
    float r[OM_MAXK];
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) r[k] = k < K ? Rb[(long)(k < K ? k : 0) * D + c] : 0.f;
    for (int n = 0; n < N; ++n) {
      float u = 0.f;
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) u += sT[n * K + k] * r[k];
      out[((long)b * N + n) * D + c] = u;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward 1
// grid B.  LDS: gamma [N*K], dt / s [N*K]
__global__ __launch_bounds__(256) void omap_bwd_pool_kernel(const float* __restrict__ Y, const float* __restrict__ cand,
                                                            const uint8_t* __restrict__ mask, const float* __restrict__ beta,
                                                            const float* __restrict__ R, const float* __restrict__ gamma,
                                                            const float* __restrict__ dout, int N, int H, int D, int K, float s, float* dR,
                                                            float* __restrict__ dcand, float* __restrict__ db) {
  extern __shared__ __align__(16) float om_smem[];
  float* sG = om_smem;
  float* sDt = sG + N * K;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* Rb = R + (long)b * K * D;
  const float* dUb = dout + (long)b * N * D;
  const float* Cb = cand + (long)b * N * D;
  float* dRb = dR + (long)b * K * D;
  for (int p = tid; p < N * K; p += 256) sG[p] = gamma[(long)b * N * K + p];
  for (int p = w; p < N * K; p += 4) {        // d gamma[n, k] = <dU[n], R[k]>
    const int n = p / K, k = p - n * K;
    float d = 0.f;
    for (int c = lane; c < D; c += 64) d += dUb[(long)n * D + c] * Rb[(long)k * D + c];
    d = wave_sum(d);
    if (lane == 0) sDt[p] = d;
  }
  __syncthreads();
  for (int n = tid; n < N; n += 256) {        // softmax backward; the 1 / s of t = C R^T / s is folded in (both uses carry it)
    float dot = 0.f;
    for (int k = 0; k < K; ++k) dot += sG[n * K + k] * sDt[n * K + k];
    for (int k = 0; k < K; ++k) sDt[n * K + k] = sG[n * K + k] * (sDt[n * K + k] - dot) / s;
  }
  __syncthreads();
  for (int c = tid; c < D; c += 256) {
    float dr[OM_MAXK], r[OM_MAXK];
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) {
      dr[k] = 0.f;
      r[k] = k < K ? Rb[(long)(k < K ? k : 0) * D + c] : 0.f;
    }
    for (int n = 0; n < N; ++n) {
      const float du = dUb[(long)n * D + c], cv = Cb[(long)n * D + c];
      float dc = 0.f;
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) {
          dr[k] += sG[n * K + k] * du + sDt[n * K + k] * cv;
          dc += sDt[n * K + k] * r[k];
        }
      dcand[((long)b * N + n) * D + c] = dc;
    }
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k)
      if (k < K) dRb[(long)k * D + c] = dr[k];
  }
  __threadfence();
  __syncthreads();                            // dR of this user is complete and visible to the workgroup
  // d beta[i, k] = <Y[i], dR[k]>, softmax backward over the heads; a padded row's scores are constants (masked_fill): db = 0
  for (int i = w; i < H; i += 4) {
    const float* y = Y + ((long)b * H + i) * D;
    float acc[OM_MAXK];
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k) acc[k] = 0.f;
    for (int c = lane; c < D; c += 64) {
      const float yv = y[c];
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) acc[k] += yv * dRb[(long)k * D + c];
    }
    const bool live = !mask || mask[(long)b * H + i];
    const float* be = beta + ((long)b * H + i) * K;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < OM_MAXK; ++k)
      if (k < K) {
        acc[k] = wave_sum(acc[k]);
        dot += be[k] * acc[k];
      }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) db[((long)b * H + i) * K + k] = live ? be[k] * (acc[k] - dot) : 0.f;
    }
  }
}

// dY[i, c] = sum_k beta[i, k] dR[k, c] + db[i, k] W[c, k] / s for the 64 columns from c0 (thread: column tid & 63, rows tid >> 6 + 4 u) -> LDS tile
// [HP][ld] (zeros outside H x D), and the same block of X beside it
template <int NB>
__device__ __forceinline__ void om_stage_dy_x(float* sdY, float* sX, int ld, const float* __restrict__ Xb, int ldf, const float* __restrict__ dRb,
                                              const float* __restrict__ W, const float* sBeta, const float* sDb, int H, int D, int K, int c0,
                                              float s, int tid) {
  const int c = tid & 63;
  const bool cl = c0 + c < D;
  float drk[OM_MAXK], wk[OM_MAXK];
#pragma unroll
  for (int k = 0; k < OM_MAXK; ++k) {
    const bool on = cl && k < K;
    drk[k] = on ? dRb[(long)k * D + c0 + c] : 0.f;
    wk[k] = on ? W[(long)(c0 + c) * K + k] / s : 0.f;
  }
  for (int i = tid >> 6; i < NB * 32; i += 4) {
    float v = 0.f, x = 0.f;
    if (cl && i < H) {
      x = Xb[(long)i * ldf + c0 + c];
#pragma unroll
      for (int k = 0; k < OM_MAXK; ++k)
        if (k < K) v += sBeta[i * K + k] * drk[k] + sDb[i * K + k] * wk[k];
    }
    sdY[i * ld + c] = v;
    sX[i * ld + c] = x;
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward 2
// grid B.  G[b] = (dS + dS^T) / s with dS = alpha o (d alpha - rowsum(alpha o d alpha)) on live keys, d alpha = dY X^T
template <int NB>
__global__ __launch_bounds__(256) void omap_bwd_dalpha_kernel(const float* __restrict__ X, int ldf, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ W, const float* __restrict__ alpha,
                                                              const float* __restrict__ beta, const float* __restrict__ dR,
                                                              const float* __restrict__ db, int H, int D, int K, float s,
                                                              float* __restrict__ G) {
  constexpr int HP = NB * 32, NT = (NB * NB + 3) / 4, SS = HP + 1;
  extern __shared__ __align__(16) float om_smem[];
  float* sdY = om_smem;                       // [HP][OM_LD]
  float* sX = sdY + HP * OM_LD;               // [HP][OM_LD]; both together hold the [HP][SS] tile afterwards
  float* sBeta = sX + HP * OM_LD;
  float* sDb = sBeta + H * K;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, half = lane >> 5;
  for (int p = tid; p < H * K; p += 256) {
    sBeta[p] = beta[(long)b * H * K + p];
    sDb[p] = db[(long)b * H * K + p];
  }
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = om_zero16();
  for (int c0 = 0; c0 < D; c0 += OM_KC) {
    __syncthreads();                          // the previous chunk has been multiplied (first trip: beta / db are staged)
    om_stage_dy_x<NB>(sdY, sX, OM_LD, X + (long)b * H * ldf, ldf, dR + (long)b * K * D, W, sBeta, sDb, H, D, K, c0, s, tid);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int tile = w + 4 * t;
      if (tile < NB * NB) {
        const float* ya = sdY + ((tile / NB) * 32 + l31) * OM_LD + half;
        const float* xb = sX + ((tile % NB) * 32 + l31) * OM_LD + half;
#pragma unroll 8
        for (int ks = 0; ks < OM_KC; ks += 2) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ya[ks], xb[ks], acc[t], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  float* sD = om_smem;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = w + 4 * t;
    if (tile < NB * NB) {
      const int ib = tile / NB, jb = tile % NB;
#pragma unroll
      for (int r = 0; r < 16; ++r) sD[(ib * 32 + om_row(r, half)) * SS + jb * 32 + l31] = acc[t][r];
    }
  }
  __syncthreads();
  const uint8_t* mb = mask ? mask + (long)b * H : nullptr;
  const float* ab = alpha + (long)b * H * H;
  for (int i = w; i < H; i += 4) {
    float* row = sD + i * SS;
    float dot = 0.f;
    for (int j = lane; j < H; j += 64) dot += ab[(long)i * H + j] * row[j];
    dot = wave_sum(dot);
    for (int j = lane; j < H; j += 64) row[j] = (!mb || mb[j]) ? ab[(long)i * H + j] * (row[j] - dot) : 0.f;
  }
  __syncthreads();
  for (int p = tid; p < H * H; p += 256) {
    const int i = p / H, j = p - i * H;
    G[(long)b * H * H + p] = (sD[i * SS + j] + sD[j * SS + i]) / s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward 3
// grid B * S.  dX[b, :, slice] (+)= dY + alpha^T dY + G X;  dwrows[b, c, k] = sum_i Y[i, c] db[i, k] / s
template <int NB>
__global__ __launch_bounds__(256) void omap_bwd_dx_kernel(const float* __restrict__ X, int ldf, const float* __restrict__ W,
                                                          const float* __restrict__ alpha, const float* __restrict__ Y,
                                                          const float* __restrict__ beta, const float* __restrict__ dR,
                                                          const float* __restrict__ db, const float* __restrict__ G, int H, int D, int K, int S,
                                                          float s, float* __restrict__ dX, int accumulate, float* __restrict__ dwrows) {
  constexpr int HP = NB * 32, NT = (NB * 2 + 3) / 4, NA = NB * 16;
  extern __shared__ __align__(16) float om_smem[];
  float* sdY = om_smem;                       // [HP][OM_KC]
  float* sX = sdY + HP * OM_KC;
  float* sBeta = sX + HP * OM_KC;
  float* sDb = sBeta + H * K;
  const int b = blockIdx.x / S, sl = blockIdx.x - b * S, c0 = sl * OM_KC;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, half = lane >> 5;
  for (int p = tid; p < H * K; p += 256) {
    sBeta[p] = beta[(long)b * H * K + p];
    sDb[p] = db[(long)b * H * K + p];
  }
  __syncthreads();
  om_stage_dy_x<NB>(sdY, sX, OM_KC, X + (long)b * H * ldf, ldf, dR + (long)b * K * D, W, sBeta, sDb, H, D, K, c0, s, tid);
  // this user's rows of dW: thread (column, head group w): heads w, w + 4, ...
  {
    const int c = c0 + lane;
    if (c < D && w < K) {
      float a4[4] = {0.f, 0.f, 0.f, 0.f};
      const float* yc = Y + (long)b * H * D + c;
#pragma unroll 4
      for (int i = 0; i < H; ++i) {
        const float y = yc[(long)i * D];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (w + 4 * q < K) a4[q] += y * sDb[i * K + w + 4 * q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (w + 4 * q < K) dwrows[((long)b * D + c) * K + w + 4 * q] = a4[q] / s;
    }
  }
  __syncthreads();
  const float* ab = alpha + (long)b * H * H;
  const float* gb = G + (long)b * H * H;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = w + 4 * t;
    if (tile < NB * 2) {
      const int ib = tile >> 1, cc = (tile & 1) * 32 + l31, i = ib * 32 + l31;
      f32x16 acc = om_zero16();
      float av[NA];
#pragma unroll
      for (int u = 0; u < NA; ++u) {          // alpha^T: A[row i][k j] = alpha[j, i]
        const int j = 2 * u + half;
        av[u] = (i < H && j < H) ? ab[(long)j * H + i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < NA; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], sdY[(2 * u + half) * OM_KC + cc], acc, 0, 0, 0);
#pragma unroll
      for (int u = 0; u < NA; ++u) {          // G is symmetric: read it along its rows
        const int j = 2 * u + half;
        av[u] = (i < H && j < H) ? gb[(long)j * H + i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < NA; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], sX[(2 * u + half) * OM_KC + cc], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int io = ib * 32 + om_row(r, half);
        if (io < H && c0 + cc < D) {
          float* o = dX + ((long)b * H + io) * D + c0 + cc;
          const float v = sdY[io * OM_KC + cc] + acc[r];
          *o = accumulate ? *o + v : v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- regulariser
// one workgroup: off[k1 * K + k2] = (W^T W)[k1, k2] off the diagonal, 0 on it; off[K * K] = Omega = ||Off||_F; loss = coef * Omega
__global__ __launch_bounds__(256) void omap_reg_fwd_kernel(const float* __restrict__ W, int D, int K, float coef, float* __restrict__ off,
                                                           float* __restrict__ loss) {
  __shared__ float sOff[OM_MAXK * OM_MAXK];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int p = w; p < K * K; p += 4) {
    const int k1 = p / K, k2 = p - k1 * K;
    float d = 0.f;
    if (k1 != k2)
      for (int r = lane; r < D; r += 64) d += W[(long)r * K + k1] * W[(long)r * K + k2];
    d = wave_sum(d);
    if (lane == 0) sOff[p] = d;
  }
  __syncthreads();
  if (w == 0) {
    float q = 0.f;
    for (int p = lane; p < K * K; p += 64) q += sOff[p] * sOff[p];
    q = wave_sum(q);
    const float omega = sqrtf(q);
    for (int p = lane; p < K * K; p += 64) off[p] = sOff[p];
    if (lane == 0) {
      off[K * K] = omega;
      *loss = coef * omega;
    }
  }
}

// dW[d, k] += g * coef * 2 * sum_k' W[d, k'] Off[k', k] / Omega   (nothing at Omega == 0: torch's gradient of the norm is zero there)
__global__ __launch_bounds__(256) void omap_reg_bwd_kernel(const float* __restrict__ W, const float* __restrict__ off, const float* __restrict__ g,
                                                           int D, int K, float coef, float* __restrict__ dW) {
  const float omega = off[K * K];
  if (omega == 0.f) return;
  const float f = g[0] * coef * 2.f / omega;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)D * K) return;
  const int d = (int)(p / K), k = (int)(p - (long)d * K);
  float a = 0.f;
  for (int q = 0; q < K; ++q) a += W[(long)d * K + q] * off[q * K + k];
  dW[p] += f * a;
}

inline int om_slices(int D) { return (D + OM_KC - 1) / OM_KC; }
inline int om_blocks(int H) { return (H + 31) / 32; }
inline bool om_sizes_ok(int B, int N, int H, int D, int K) { return B >= 1 && N >= 1 && H >= 1 && D >= 1 && K >= 1; }
inline bool om_supported(int B, int N, int H, int D, int K) {
  return H <= OM_MAXH && K <= OM_MAXK && (long)B * om_slices(D) <= 0x7fffffffL && ((long)H * K + (long)N * K) * 4 <= OM_LDS_BYTES / 4 &&
         (long)D * K <= 0x7fffffffL;
}

}  // namespace

extern "C" int nnr_omap_ws_floats(int B, int N, int H, int D, int K) {
  if (!om_sizes_ok(B, N, H, D, K)) return NNR_ERR_ARG;
  if (!om_supported(B, N, H, D, K)) return NNR_ERR_UNSUPPORTED;
  const long fwd = (long)B * om_slices(D) * H * K;
  const long bwd = (long)B * K * D + (long)B * H * K + (long)B * H * H + (long)B * D * K;
  const long n = fwd > bwd ? fwd : bwd;
  return n > 0x7fffffffL ? NNR_ERR_UNSUPPORTED : (int)n;
}

extern "C" int nnr_omap_fwd(const float* hist, int ldf, const float* cand, const uint8_t* mask, const float* W, int B, int N, int H, int D, int K,
                            float* alpha, float* Y, float* beta, float* R, float* gamma, float* out, float* ws, hipStream_t stream) {
  if (!hist || !cand || !W || !alpha || !Y || !beta || !R || !gamma || !out || !ws || !om_sizes_ok(B, N, H, D, K) || ldf < D) return NNR_ERR_ARG;
  if (nnr_omap_ws_floats(B, N, H, D, K) < 0) return NNR_ERR_UNSUPPORTED;
  const int NB = om_blocks(H), HP = NB * 32, S = om_slices(D);
  const float s = sqrtf((float)D);
  const size_t lds1 = (size_t)HP * (OM_LD > HP + 1 ? OM_LD : HP + 1) * 4;
  const size_t lds2 = ((size_t)HP * OM_LD + (size_t)OM_KC * K) * 4;
  const size_t lds3 = ((size_t)H * K + (size_t)N * K) * 4;
#define OM_L1(NBV) hipLaunchKernelGGL((omap_alpha_kernel<NBV>), dim3((unsigned)B), dim3(256), lds1, stream, hist, ldf, mask, H, D, s, alpha)
#define OM_L2(NBV) \
  hipLaunchKernelGGL((omap_mix_kernel<NBV>), dim3((unsigned)(B * S)), dim3(256), lds2, stream, hist, ldf, (const float*)alpha, W, H, D, K, S, Y, ws)
  if (NB == 1) OM_L1(1); else if (NB == 2) OM_L1(2); else OM_L1(3);
  NNR_CHECK_LAUNCH();
  if (NB == 1) OM_L2(1); else if (NB == 2) OM_L2(2); else OM_L2(3);
  NNR_CHECK_LAUNCH();
#undef OM_L1
#undef OM_L2
  hipLaunchKernelGGL(omap_pool_kernel, dim3((unsigned)B), dim3(256), lds3, stream, (const float*)Y, cand, mask, (const float*)ws, N, H, D, K, S, s,
                     beta, R, gamma, out);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_omap_bwd(const float* hist, int ldf, const float* cand, const uint8_t* mask, const float* W, const float* alpha, const float* Y,
                            const float* beta, const float* R, const float* gamma, const float* dout, int B, int N, int H, int D, int K,
                            float* dhist, int dhist_accumulate, float* dcand, float* dW_accum, float* ws, hipStream_t stream) {
  if (!hist || !cand || !W || !alpha || !Y || !beta || !R || !gamma || !dout || !dhist || !dcand || !dW_accum || !ws ||
      !om_sizes_ok(B, N, H, D, K) || ldf < D)
    return NNR_ERR_ARG;
  if (nnr_omap_ws_floats(B, N, H, D, K) < 0) return NNR_ERR_UNSUPPORTED;
  const int NB = om_blocks(H), HP = NB * 32, S = om_slices(D);
  const float s = sqrtf((float)D);
  float* dR = ws;
  float* db = dR + (long)B * K * D;
  float* G = db + (long)B * H * K;
  float* rows = G + (long)B * H * H;
  const size_t lds1 = (size_t)2 * N * K * 4;
  const size_t lds2 = ((size_t)2 * HP * OM_LD + (size_t)2 * H * K) * 4;
  const size_t lds3 = ((size_t)2 * HP * OM_KC + (size_t)2 * H * K) * 4;
  if (lds2 > (size_t)OM_LDS_BYTES || lds3 > (size_t)OM_LDS_BYTES) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(omap_bwd_pool_kernel, dim3((unsigned)B), dim3(256), lds1, stream, Y, cand, mask, beta, R, gamma, dout, N, H, D, K, s, dR, dcand,
                     db);
  NNR_CHECK_LAUNCH();
#define OM_L2(NBV)                                                                                                                            \
  hipLaunchKernelGGL((omap_bwd_dalpha_kernel<NBV>), dim3((unsigned)B), dim3(256), lds2, stream, hist, ldf, mask, W, alpha, beta, (const float*)dR, \
                     (const float*)db, H, D, K, s, G)
#define OM_L3(NBV)                                                                                                                             \
  hipLaunchKernelGGL((omap_bwd_dx_kernel<NBV>), dim3((unsigned)(B * S)), dim3(256), lds3, stream, hist, ldf, W, alpha, Y, beta, (const float*)dR, \
                     (const float*)db, (const float*)G, H, D, K, S, s, dhist, dhist_accumulate, rows)
  if (NB == 1) OM_L2(1); else if (NB == 2) OM_L2(2); else OM_L2(3);
  NNR_CHECK_LAUNCH();
  if (NB == 1) OM_L3(1); else if (NB == 2) OM_L3(2); else OM_L3(3);
  NNR_CHECK_LAUNCH();
#undef OM_L2
#undef OM_L3
  const long n = (long)D * K;
  hipLaunchKernelGGL(partial_rows_sum_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const float*)rows, B, n, dW_accum);   // backward 4
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_omap_reg_fwd(const float* W, int D, int K, float coef, float* off, float* loss, hipStream_t stream) {
  if (!W || !off || !loss || D < 1 || K < 1) return NNR_ERR_ARG;
  if (K > OM_MAXK) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(omap_reg_fwd_kernel, dim3(1), dim3(256), 0, stream, W, D, K, coef, off, loss);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_omap_reg_bwd(const float* W, const float* off, const float* gup, int D, int K, float coef, float* dW_accum, hipStream_t stream) {
  if (!W || !off || !gup || !dW_accum || D < 1 || K < 1) return NNR_ERR_ARG;
  if (K > OM_MAXK || (long)D * K > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  const long n = (long)D * K;
  hipLaunchKernelGGL(omap_reg_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, W, off, gup, D, K, coef, dW_accum);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
