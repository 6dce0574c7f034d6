// Candidate-aware additive attention: the CATT user encoder (userEncoders.py:213-220, ReLU) and layers.CandidateAttention /
// layers.MultipleCandidateAttention (layers.py:225-232, 254-262, tanh).  Per sample b, query n and feature slot h:
//   a[n,h]   = w2 . act(P[b,n,:] + Q[b,h,:])            P = query projection + bias [B*N, A], Q = feature projection [B*H, A] (two GEMMs)
//   alpha[n] = softmax_h(mask[b,h] ? a[n,h] : -1e9)     (a sample without any live slot: uniform over ALL H slots, as the reference)
//   out[n,:] = sum_h alpha[n,h] * feat[b,h,:]
// The reference materialises cat([query, feature]) as [B, N, H, 2D] and the hidden tensor [B, N, H, A]; here neither exists: the
// activations are recomputed from P and Q in the backward pass.  The bias of the score (affine2.bias of CATT) shifts every live score of a
// row by the same amount: it cannot change alpha and its gradient is exactly zero, so it is not an argument.
//
// Work split (same access pattern as sue_intra_* in misc.hip: the N queries of a sample all read that sample's [H, D] features and [H, A]
// keys; 256-thread workgroups because larger ones lose CUs to the weight-gradient GEMMs of the other stream):
//   forward      one workgroup per (sample, slice of 64 column groups): Q[b] (H x A, 40 KB at H = 50, A = 200) is staged in LDS once for the N
//                queries, thread (n, h) computes one score, one wave per query does the softmax, then the four waves share the H feature
//                rows of the slice (16-byte lanes, 4 rows in flight) and wave 0 adds the four partial sums in wave order.
//   backward 1   one workgroup per (sample, query), the N workgroups of a sample on one XCD: d alpha (wave per feature row), softmax
//                backward -> da (workspace), then thread k: dP[b,n,k] and this workgroup's own row of the dw2 partial sums.
//   backward 2   per sample: 64-column-group slices write dfeat[b,h,:] = sum_n alpha[n,h] dout[n,:] (each row once), four more workgroups
//                write dQ[b,h,:] = w2 * sum_n da[n,h] act'(P[n] + Q[h]).
//   dw2          the per-workgroup rows are summed by nnr_colsum's fixed-order reduction: no arrival-order float atomics anywhere, the
//                same inputs give the same bits.
#include "common.h"

namespace {

constexpr int CA_RELU = 1, CA_TANH = 2;          // nnr_gemm_args.act numbering
constexpr int CA_NQ = 8;                         // queries per register chunk
constexpr int CA_LDS_BYTES = 64 * 1024;          // dynamic LDS a launch may ask for without an attribute


// activation and its derivative at z
__device__ __forceinline__ void ca_act_grad(float z, int act, float* a, float* d) {
  if (act == CA_TANH) {
    const float t = tanhf(z);
    *a = t; *d = 1.f - t * t;
  } else {
    *a = fmaxf(z, 0.f); *d = z > 0.f ? 1.f : 0.f;
  }
}

// LDS floats of the forward kernel in front of its small arrays: Q[b] with an odd row stride (thread (n, h) walks row h: conflict-free), or
// without it the partial sums of waves 1..3 (which reuse the region once the scores are done)
__host__ __device__ inline int ca_fwd_region(bool qlds, int H, int A, int V) {
  const int red = 3 * CA_NQ * 64 * V, q = qlds ? H * (A | 1) : 0;
  return ((q > red ? q : red) + 3) & ~3;
}

template <bool QLDS, int V>
__global__ __launch_bounds__(256) void cand_attn_fwd_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const float* __restrict__ w2, const float* __restrict__ feat, int ldf,
                                                            const uint8_t* __restrict__ mask, int N, int H, int A, int D, int act, int S,
                                                            float* __restrict__ alpha, float* __restrict__ out) {
  typedef typename vec_t<V>::type vec;
  extern __shared__ __align__(16) float ca_smem[];
  const int b = blockIdx.x / S, slice = blockIdx.x - b * S;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int As = A | 1;
  float* sQ = ca_smem;
  vec* red = reinterpret_cast<vec*>(ca_smem);
  float* sP = ca_smem + ca_fwd_region(QLDS, H, A, V);
  float* sw2 = sP + N * A;
  float* sal = sw2 + A;
  const float* Qb = Q + (long)b * H * A;
  if (QLDS)
    for (int i = tid; i < H * A; i += 256) {
      const int h = i / A;
      sQ[h * As + (i - h * A)] = Qb[i];
    }
  for (int i = tid; i < N * A; i += 256) sP[i] = P[(long)b * N * A + i];
  for (int i = tid; i < A; i += 256) sw2[i] = w2[i];
  __syncthreads();
  // scores: thread (n, h)
  for (int p = tid; p < N * H; p += 256) {
    const int n = p / H, h = p - n * H;
    const float* q = QLDS ? sQ + h * As : Qb + (long)h * A;
    const float* pr = sP + n * A;
    float s = 0.f;
    if (act == CA_TANH)
      for (int k = 0; k < A; ++k) s += sw2[k] * tanhf(pr[k] + q[k]);
    else
      for (int k = 0; k < A; ++k) s += sw2[k] * fmaxf(pr[k] + q[k], 0.f);
    if (mask && !mask[(long)b * H + h]) s = -1e9f;
    sal[p] = s;
  }
  __syncthreads();
  // softmax over h: one wave per query
  for (int n = w; n < N; n += 4) {
    float* row = sal + n * H;
    float m = -INFINITY;
    for (int h = lane; h < H; h += 64) m = fmaxf(m, row[h]);
    m = wave_max(m);
    float sm = 0.f;
    for (int h = lane; h < H; h += 64) {
      const float e = expf(row[h] - m);
      row[h] = e;
      sm += e;
    }
    sm = wave_sum(sm);
    for (int h = lane; h < H; h += 64) {
      const float v = row[h] / sm;
      row[h] = v;
      if (slice == 0) alpha[((long)b * N + n) * H + h] = v;
    }
  }
  __syncthreads();
  // out[n, cols] = sum_h alpha[n, h] feat[b, h, cols]: wave w takes the rows h = w, w + 4, ...
  const int ncol = D / V, c = slice * 64 + lane;
  const bool live = c < ncol;
  const float* fb = feat + (long)b * H * ldf + (long)c * V;
  for (int n0 = 0; n0 < N; n0 += CA_NQ) {
    vec acc[CA_NQ];
#pragma unroll
    for (int j = 0; j < CA_NQ; ++j) acc[j] = vzero<V>();
    for (int h0 = w; h0 < H; h0 += 16) {
      vec f[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) f[u] = (live && h0 + 4 * u < H) ? *reinterpret_cast<const vec*>(fb + (long)(h0 + 4 * u) * ldf) : vzero<V>();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (h0 + 4 * u < H) {
#pragma unroll
          for (int j = 0; j < CA_NQ; ++j)
            if (n0 + j < N) acc[j] += sal[(n0 + j) * H + h0 + 4 * u] * f[u];
        }
      }
    }
    if (w > 0) {
#pragma unroll
      for (int j = 0; j < CA_NQ; ++j) red[((w - 1) * CA_NQ + j) * 64 + lane] = acc[j];
    }
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
      for (int j = 0; j < CA_NQ; ++j)
        if (n0 + j < N) {
          vec r = acc[j];
#pragma unroll
          for (int q = 0; q < 3; ++q) r += red[(q * CA_NQ + j) * 64 + lane];
          *reinterpret_cast<vec*>(out + ((long)b * N + n0 + j) * D + (long)c * V) = r;
        }
    }
    __syncthreads();
  }
}

// workgroup id -> (sample, query) with every workgroup of a sample on ONE XCD (consecutive ids go to different XCDs, whose L2s do not
// share; see sue_xcd_map in misc.hip for what that measured)
__device__ __forceinline__ bool ca_xcd_map(int id, int B, int per_sample, int* b, int* i) {
  const int x = id & 7, slot = id >> 3;
  *b = (slot / per_sample) * 8 + x;
  *i = slot % per_sample;
  return *b < B;
}

// backward 1, grid ceil(B / 8) * 8 * N: da[b, n, :] (workspace), dP[b, n, :] and the workgroup's row of the dw2 partial sums
template <int V>
__global__ __launch_bounds__(256) void cand_attn_bwd_da_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                               const float* __restrict__ w2, const float* __restrict__ feat, int ldf,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ alpha,
                                                               const float* __restrict__ dout, int B, int N, int H, int A, int D, int act,
                                                               float* __restrict__ da_ws, float* __restrict__ dP, float* __restrict__ dw2_rows) {
  typedef typename vec_t<V>::type vec;
  extern __shared__ __align__(16) float ca_smem[];
  float* sal = ca_smem;
  float* sdl = sal + H;
  float* sda = sdl + H;
  int b, ni;
  if (!ca_xcd_map(blockIdx.x, B, N, &b, &ni)) return;
  const int bn = b * N + ni, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int j = tid; j < H; j += 256) sal[j] = alpha[(long)bn * H + j];
  // d alpha[h] = <dout[b, n], feat[b, h]>: 4 rows per wave and trip, their loads in flight together
  const int ncol = D / V;
  const float* fb = feat + (long)b * H * ldf;
  const float* dr = dout + (long)bn * D;
  for (int j0 = w; j0 < H; j0 += 16) {
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    const float* fr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) fr[u] = fb + (long)min(j0 + 4 * u, H - 1) * ldf;
    for (int x = lane; x < ncol; x += 64) {
      const vec d = *reinterpret_cast<const vec*>(dr + (long)x * V);
      vec f[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) f[u] = *reinterpret_cast<const vec*>(fr[u] + (long)x * V);
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u] += vdot(d, f[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = wave_sum(p[u]);
      if (lane == 0 && j0 + 4 * u < H) sdl[j0 + 4 * u] = t;
    }
  }
  __syncthreads();
  // softmax backward; a masked slot's score is a constant (masked_fill): no gradient
  float dot = 0.f;
  for (int j = lane; j < H; j += 64) dot += sal[j] * sdl[j];
  dot = wave_sum(dot);                                  // (every wave sums in the same order: one value)
  for (int j = tid; j < H; j += 256) {
    const float v = (!mask || mask[(long)b * H + j]) ? sal[j] * (sdl[j] - dot) : 0.f;
    sda[j] = v;
    da_ws[(long)bn * H + j] = v;
  }
  __syncthreads();
  // dP[k] = w2[k] sum_h da[h] act'(P[k] + Q[h, k]);  dw2 row[k] = sum_h da[h] act(P[k] + Q[h, k])
  for (int k = tid; k < A; k += 256) {
    const float p = P[(long)bn * A + k];
    const float* qb = Q + (long)b * H * A + k;
    float accP = 0.f, accW = 0.f;
    for (int j = 0; j < H; j += 8) {
      float q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] = qb[(long)min(j + u, H - 1) * A];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j + u < H) {
          float a, d;
          ca_act_grad(p + q[u], act, &a, &d);
          accW += sda[j + u] * a;
          accP += sda[j + u] * d;
        }
    }
    dP[(long)bn * A + k] = w2[k] * accP;
    dw2_rows[(long)bn * A + k] = accW;
  }
}

// backward 2, grid B * (S + ZQ): slices y < S -> dfeat[b, h, cols] (+)= sum_n alpha[b, n, h] dout[b, n, cols], every row written once per
// chunk of 8 queries (read first only when it accumulates); y >= S -> part y - S of dQ[b, h, :] = w2 * sum_n da[b, n, h] act'(P[b, n] + Q[b, h]),
// one element per thread and trip with 4 independent loads of Q in flight (as one workgroup per sample walking the H rows in turn this part
// was latency-bound: 38 us of the launch at batch 64)
constexpr int CA_ZQ = 4;
template <int V>
__global__ __launch_bounds__(256) void cand_attn_bwd_dx_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                               const float* __restrict__ w2, const float* __restrict__ alpha,
                                                               const float* __restrict__ da_ws, const float* __restrict__ dout, int N, int H,
                                                               int A, int D, int act, int S, float* __restrict__ dQ, float* __restrict__ dfeat,
                                                               int accumulate) {
  typedef typename vec_t<V>::type vec;
  extern __shared__ __align__(16) float ca_smem[];
  const int b = blockIdx.x / (S + CA_ZQ), y = blockIdx.x - b * (S + CA_ZQ);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool qpart = y >= S;
  const float* src = (qpart ? da_ws : alpha) + (long)b * N * H;
  float* sP = ca_smem + N * H;
  for (int i = tid; i < N * H; i += 256) ca_smem[i] = src[i];
  if (qpart)
    for (int i = tid; i < N * A; i += 256) sP[i] = P[(long)b * N * A + i];
  __syncthreads();
  if (qpart) {
    const int total = H * A, chunk = (total + CA_ZQ - 1) / CA_ZQ;
    const int i0 = (y - S) * chunk, i1 = min(total, i0 + chunk);
    const float* Qb = Q + (long)b * total;
    float* dQb = dQ + (long)b * total;
    for (int i = i0 + tid; i < i1; i += 1024) {
      float q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = i + 256 * u < i1 ? Qb[i + 256 * u] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = i + 256 * u;
        if (idx < i1) {
          const int h = idx / A, k = idx - h * A;
          float acc = 0.f;
          for (int n = 0; n < N; ++n) {
            float a, d;
            ca_act_grad(sP[n * A + k] + q[u], act, &a, &d);
            acc += ca_smem[n * H + h] * d;
          }
          dQb[idx] = w2[k] * acc;
        }
      }
    }
    return;
  }
  const int ncol = D / V, c = y * 64 + lane;
  if (c >= ncol) return;
  for (int n0 = 0; n0 < N; n0 += CA_NQ) {
    vec dv[CA_NQ];
#pragma unroll
    for (int j = 0; j < CA_NQ; ++j) dv[j] = n0 + j < N ? *reinterpret_cast<const vec*>(dout + ((long)b * N + n0 + j) * D + (long)c * V) : vzero<V>();
    for (int h = w; h < H; h += 4) {
      vec acc = vzero<V>();
#pragma unroll
      for (int j = 0; j < CA_NQ; ++j)
        if (n0 + j < N) acc += ca_smem[(n0 + j) * H + h] * dv[j];
      vec* o = reinterpret_cast<vec*>(dfeat + ((long)b * H + h) * D + (long)c * V);
      if (n0 || accumulate) acc += *o;
      *o = acc;
    }
  }
}


}  // namespace

extern "C" int nnr_cand_attn_ws_floats(int B, int N, int H, int A) {
  if (B < 1 || N < 1 || H < 1 || A < 1) return NNR_ERR_ARG;
  const long n = (long)B * N * H + (long)B * N * A + nnr_slot_workspace_floats(A);
  return n > 0x7fffffffL ? NNR_ERR_UNSUPPORTED : (int)n;
}

extern "C" int nnr_cand_attn_fwd(const float* P, const float* Q, const float* w2, const float* feat, int ldf, const uint8_t* mask, int B, int N,
                                 int H, int A, int D, int act, float* alpha, float* out, hipStream_t stream) {
  if (!P || !Q || !w2 || !feat || !alpha || !out || B < 1 || N < 1 || H < 1 || A < 1 || D < 1 || ldf < D || (act != CA_RELU && act != CA_TANH))
    return NNR_ERR_ARG;
  const int V = (!(D & 3) && !(ldf & 3) && al16(feat) && al16(out)) ? 4 : 1;
  const int S = (D / V + 63) / 64;
  const long small = (long)N * A + A + (long)N * H;
  if (small * 4 > CA_LDS_BYTES) return NNR_ERR_UNSUPPORTED;
  bool qlds = (long)H * (A | 1) * 4 <= CA_LDS_BYTES;
  long floats = ca_fwd_region(qlds, H, A, V) + small;
  if (qlds && floats * 4 > CA_LDS_BYTES) {
    qlds = false;                                       // Q[b] does not fit beside the rest: the scores read it from global memory
    floats = ca_fwd_region(false, H, A, V) + small;
  }
  if (floats * 4 > CA_LDS_BYTES) return NNR_ERR_UNSUPPORTED;
  if ((long)B * S > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(B * S)), block(256);
  const size_t lds = (size_t)floats * 4;
#define CA_FWD(QL, VV) \
  hipLaunchKernelGGL((cand_attn_fwd_kernel<QL, VV>), grid, block, lds, stream, P, Q, w2, feat, ldf, mask, N, H, A, D, act, S, alpha, out)
  if (qlds) { if (V == 4) CA_FWD(true, 4); else CA_FWD(true, 1); }
  else { if (V == 4) CA_FWD(false, 4); else CA_FWD(false, 1); }
#undef CA_FWD
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_cand_attn_bwd(const float* P, const float* Q, const float* w2, const float* feat, int ldf, const uint8_t* mask,
                                 const float* alpha, const float* dout, int B, int N, int H, int A, int D, int act, float* dP, float* dQ,
                                 float* dfeat, int dfeat_accumulate, float* ws, float* dw2, hipStream_t stream) {
  if (!P || !Q || !w2 || !feat || !alpha || !dout || !dP || !dQ || !dfeat || !ws || !dw2 || B < 1 || N < 1 || H < 1 || A < 1 || D < 1 ||
      ldf < D || (act != CA_RELU && act != CA_TANH))
    return NNR_ERR_ARG;
  if (nnr_cand_attn_ws_floats(B, N, H, A) < 0) return NNR_ERR_UNSUPPORTED;
  const int V = (!(D & 3) && !(ldf & 3) && al16(feat) && al16(dout) && al16(dfeat)) ? 4 : 1;
  const int S = (D / V + 63) / 64;
  const long lds2 = ((long)N * H + (long)N * A) * 4;
  if (3L * H * 4 > CA_LDS_BYTES || lds2 > CA_LDS_BYTES || (long)H * A > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  const long g1 = (long)((B + 7) / 8) * 8 * N, g2 = (long)B * (S + CA_ZQ);
  if (g1 > 0x7fffffffL || g2 > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  float* da_ws = ws;
  float* rows = ws + (long)B * N * H;
  float* slots = rows + (long)B * N * A;
  if (V == 4)
    hipLaunchKernelGGL((cand_attn_bwd_da_kernel<4>), dim3((unsigned)g1), dim3(256), (size_t)3 * H * 4, stream, P, Q, w2, feat, ldf, mask, alpha,
                       dout, B, N, H, A, D, act, da_ws, dP, rows);
  else
    hipLaunchKernelGGL((cand_attn_bwd_da_kernel<1>), dim3((unsigned)g1), dim3(256), (size_t)3 * H * 4, stream, P, Q, w2, feat, ldf, mask, alpha,
                       dout, B, N, H, A, D, act, da_ws, dP, rows);
  NNR_CHECK_LAUNCH();
  if (V == 4)
    hipLaunchKernelGGL((cand_attn_bwd_dx_kernel<4>), dim3((unsigned)g2), dim3(256), (size_t)lds2, stream, P, Q, w2, alpha,
                       (const float*)da_ws, dout, N, H, A, D, act, S, dQ, dfeat, dfeat_accumulate);
  else
    hipLaunchKernelGGL((cand_attn_bwd_dx_kernel<1>), dim3((unsigned)g2), dim3(256), (size_t)lds2, stream, P, Q, w2, alpha,
                       (const float*)da_ws, dout, N, H, A, D, act, S, dQ, dfeat, dfeat_accumulate);
  NNR_CHECK_LAUNCH();
  // dw2[k] += sum over the B*N workgroup rows, in nnr_colsum's fixed order (own slot rows, then the slot reduction)
  return nnr_colsum(rows, A, nullptr, B * N, A, dw2, slots, stream);
}
