// Segmented candidate pool in GEMV form: the intra-cluster attention of SUE_wo_GCN (variantEncoders.py:377-381).  A translation unit of its own so
// that csrc/misc.hip -- and with it every kernel of the CNE + SUE step -- compiles to the object it always did.  SUE_MAXH / SUE_MAXC, sue_members
// and sue_xcd_map are misc.hip's (sue_intra_*), restated here: the limits and the work split are the same on purpose.
#include "common.h"

namespace {

constexpr int SUE_MAXH = 64, SUE_MAXC = 32;

// cluster-sorted member list of one user: ccnt / cstart per cluster, order[] = the items cluster by cluster, ascending inside a cluster
__device__ __forceinline__ void sue_members(const int* cid, int Hn, int C, int* ccnt, int* cstart, int* order) {
  const int tid = threadIdx.x;
  if (tid < C) {
    int n = 0;
    for (int j = 0; j < Hn; ++j) n += (cid[j] == tid);
    ccnt[tid] = n;
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c < C; ++c) { cstart[c] = acc; acc += ccnt[c]; }
  }
  __syncthreads();
  if (tid < C) {
    int k = cstart[tid];
    for (int j = 0; j < Hn; ++j) if (cid[j] == tid) order[k++] = j;
  }
  __syncthreads();
}

// workgroup id -> (XCD x = id & 7, slot = id >> 3) -> user b = 8 (slot / per_user) + x: every workgroup of a user runs on ONE XCD, whose L2 then
// holds the user's [Hn, D] rows once for its N readers (measured for sue_intra_*, see misc.hip)
__device__ __forceinline__ bool sue_xcd_map(int id, int B, int per_user, int* b, int* w) {
  const int x = id & 7, slot = id >> 3;
  *b = (slot / per_user) * 8 + x;
  *w = slot % per_user;
  return *b < B;
}

// The key projection's bias adds one constant to every score of a (user, candidate) and cancels in each segment softmax, so
// K(x_h) . q_n = x_h . (W_K^T q_n) = x_h . u_n  and the [B Hn, A] key buffer never exists:
// s_h = scale <x_h, u_n>,  alpha = softmax of s within each cluster,  feat_c = sum_{h in c} alpha_h x_h.
// Out-of-range cluster ids are clamped into [0, C) (torch_scatter would raise; here they must not become addresses).
__device__ __forceinline__ void seg_load_cid(const long* __restrict__ cidx, int b, int Hn, int C, int* cid) {
  for (int j = threadIdx.x; j < Hn; j += blockDim.x) cid[j] = (int)min(max(cidx[(long)b * Hn + j], 0L), (long)(C - 1));
}
// out[j] = mul * <other[(ridx ? ridx[j] : 0), :], xb[j, :]> for the Hn rows of one user, by the 4 waves of a 256-thread workgroup: 4 rows per
// wave and trip with float4 lanes when the rows are 16-byte aligned (the dalpha loop of sue_intra_bwd_ds_kernel)
__device__ __forceinline__ void seg_row_dots(const float* __restrict__ xb, const float* __restrict__ other, const int* ridx, int Hn, int D,
                                             float mul, float* out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  if (!(D & 3) && !((reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(other)) & 15)) {
    const int D4 = D >> 2;
    for (int j0 = w; j0 < Hn; j0 += 4 * nw) {
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      const f32x4* a[4];
      const f32x4* c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = min(j0 + nw * u, Hn - 1);
        a[u] = reinterpret_cast<const f32x4*>(other + (ridx ? (long)ridx[j] * D : 0L));
        c[u] = reinterpret_cast<const f32x4*>(xb + (long)j * D);
      }
      for (int x = lane; x < D4; x += 64) {
        f32x4 av[4], cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { av[u] = a[u][x]; cv[u] = c[u][x]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] += av[u][0] * cv[u][0] + av[u][1] * cv[u][1] + av[u][2] * cv[u][2] + av[u][3] * cv[u][3];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float t = wave_sum(p[u]);
        if (lane == 0 && j0 + nw * u < Hn) out[j0 + nw * u] = t * mul;
      }
    }
  } else {
    for (int j = w; j < Hn; j += nw) {
      const float* ar = other + (ridx ? (long)ridx[j] * D : 0L);
      const float* cr = xb + (long)j * D;
      float p = 0.f;
      for (int x = lane; x < D; x += 64) p += ar[x] * cr[x];
      p = wave_sum(p);
      if (lane == 0) out[j] = p * mul;
    }
  }
}

// forward: one workgroup per (b, n), the N workgroups of a user on one XCD (sue_xcd_map): scores over D, segment softmax, then every thread
// walks the cluster-sorted member list once per column it owns (members in ascending h inside a cluster, as the forward above).
__global__ __launch_bounds__(256) void sue_seg_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                                const long* __restrict__ cidx, int B, int N, int Hn, int C, int D, float scale,
                                                                float* __restrict__ alpha, float* __restrict__ feat) {
  __shared__ float sc[SUE_MAXH], al[SUE_MAXH], cmax[SUE_MAXC], csum[SUE_MAXC];
  __shared__ int cid[SUE_MAXH], order[SUE_MAXH], ccnt[SUE_MAXC], cstart[SUE_MAXC];
  int b, ni;
  if (!sue_xcd_map(blockIdx.x, B, N, &b, &ni)) return;
  const int bn = b * N + ni, tid = threadIdx.x;
  seg_load_cid(cidx, b, Hn, C, cid);
  const float* xb = x + (long)b * Hn * D;
  seg_row_dots(xb, u + (long)bn * D, nullptr, Hn, D, scale, sc);
  __syncthreads();
  sue_members(cid, Hn, C, ccnt, cstart, order);
  if (tid < C) {
    float m = -INFINITY;
    for (int k = 0; k < ccnt[tid]; ++k) m = fmaxf(m, sc[order[cstart[tid] + k]]);
    float sm = 0.f;
    for (int k = 0; k < ccnt[tid]; ++k) sm += expf(sc[order[cstart[tid] + k]] - m);
    cmax[tid] = m; csum[tid] = sm;
  }
  __syncthreads();
  for (int j = tid; j < Hn; j += 256) {
    const float v = expf(sc[j] - cmax[cid[j]]) / csum[cid[j]];
    al[j] = v;
    alpha[(long)bn * Hn + j] = v;
  }
  __syncthreads();
  const int total = cstart[C - 1] + ccnt[C - 1];         // == Hn: every item sits in one cluster
  for (int col = tid; col < D; col += 256) {
    const float* gb = xb + col;
    float* fo = feat + (long)bn * C * D + col;
    for (int c = 0; c < C; ++c)
      if (ccnt[c] == 0) fo[(long)c * D] = 0.f;            // empty cluster -> exactly 0, as scatter_sum
    int cur = cid[order[0]];
    float acc = 0.f;
    for (int p0 = 0; p0 < total; p0 += 8) {
      int jj[8];
      float gv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        jj[t] = order[min(p0 + t, total - 1)];
        gv[t] = gb[(long)jj[t] * D];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (p0 + t < total) {
          const int cl = cid[jj[t]];
          if (cl != cur) {
            fo[(long)cur * D] = acc;
            acc = 0.f;
            cur = cl;
          }
          acc += al[jj[t]] * gv[t];
        }
      }
    }
    fo[(long)cur * D] = acc;
  }
}

// backward part 1, one workgroup per (b, n): dalpha_h = <dfeat[c(h)], x_h>, the segment-softmax backward -> ds[b, n, :] (scaled; workspace)
// and du[b, n, :] = sum_h ds_h x_h, h ascending.
__global__ __launch_bounds__(256) void sue_seg_pool_bwd_ds_kernel(const float* __restrict__ x, const long* __restrict__ cidx,
                                                                   const float* __restrict__ alpha, const float* __restrict__ dfeat, int B,
                                                                   int N, int Hn, int C, int D, float scale, float* __restrict__ ds_ws,
                                                                   float* __restrict__ du) {
  __shared__ float al[SUE_MAXH], da[SUE_MAXH], ds[SUE_MAXH], csum[SUE_MAXC];
  __shared__ int cid[SUE_MAXH];
  int b, ni;
  if (!sue_xcd_map(blockIdx.x, B, N, &b, &ni)) return;
  const int bn = b * N + ni, tid = threadIdx.x;
  seg_load_cid(cidx, b, Hn, C, cid);
  for (int j = tid; j < Hn; j += 256) al[j] = alpha[(long)bn * Hn + j];
  __syncthreads();
  const float* xb = x + (long)b * Hn * D;
  seg_row_dots(xb, dfeat + (long)bn * C * D, cid, Hn, D, 1.f, da);
  __syncthreads();
  if (tid < C) {
    float sm = 0.f;
    for (int j = 0; j < Hn; ++j) if (cid[j] == tid) sm += al[j] * da[j];
    csum[tid] = sm;
  }
  __syncthreads();
  for (int j = tid; j < Hn; j += 256) {
    const float v = al[j] * (da[j] - csum[cid[j]]) * scale;
    ds[j] = v;
    ds_ws[(long)bn * Hn + j] = v;
  }
  __syncthreads();
  for (int col = tid; col < D; col += 256) {
    float acc = 0.f;
    int j = 0;
    for (; j + 8 <= Hn; j += 8) {
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = xb[(long)(j + t) * D + col];
#pragma unroll
      for (int t = 0; t < 8; ++t) acc += ds[j + t] * v[t];
    }
    for (; j < Hn; ++j) acc += ds[j] * xb[(long)j * D + col];
    du[(long)bn * D + col] = acc;
  }
}

// backward part 2, grid (B, ceil(D/256), Z): dx[b, h, cols] = sum_n (alpha[b,n,h] dfeat[b,n,c(h),cols] + ds[b,n,h] u[b,n,cols]), n ascending;
// every row belongs to exactly one cluster and blockIdx.z deals the clusters, so each element is written exactly once (no read-modify-write).
__global__ __launch_bounds__(256) void sue_seg_pool_bwd_dx_kernel(const float* __restrict__ u, const long* __restrict__ cidx,
                                                                   const float* __restrict__ alpha, const float* __restrict__ dfeat,
                                                                   const float* __restrict__ ds_ws, int N, int Hn, int C, int D,
                                                                   float* __restrict__ dx) {
  __shared__ float al[8][SUE_MAXH], ds[8][SUE_MAXH];
  __shared__ int cid[SUE_MAXH], order[SUE_MAXH], ccnt[SUE_MAXC], cstart[SUE_MAXC];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < N * Hn; i += 256) {
    const int n = i / Hn, j = i - n * Hn;
    al[n][j] = alpha[((long)b * N + n) * Hn + j];
    ds[n][j] = ds_ws[((long)b * N + n) * Hn + j];
  }
  seg_load_cid(cidx, b, Hn, C, cid);
  __syncthreads();
  sue_members(cid, Hn, C, ccnt, cstart, order);
  const int col = blockIdx.y * 256 + tid;
  if (col >= D) return;
  float uv[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) uv[n] = n < N ? u[((long)b * N + n) * D + col] : 0.f;
  const int Z = gridDim.z;
  int c = blockIdx.z;
  while (c < C && ccnt[c] == 0) c += Z;
  float nx[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) nx[n] = (n < N && c < C) ? dfeat[(((long)b * N + n) * C + c) * D + col] : 0.f;
  while (c < C) {
    float dv[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) dv[n] = nx[n];
    int cn = c + Z;
    while (cn < C && ccnt[cn] == 0) cn += Z;
#pragma unroll
    for (int n = 0; n < 8; ++n) nx[n] = (n < N && cn < C) ? dfeat[(((long)b * N + n) * C + cn) * D + col] : 0.f;
    for (int k = 0; k < ccnt[c]; ++k) {
      const int j = order[cstart[c] + k];
      float acc = 0.f;
#pragma unroll
      for (int n = 0; n < 8; ++n) if (n < N) acc += al[n][j] * dv[n] + ds[n][j] * uv[n];      // rows n >= N of the LDS tables are never written
      dx[((long)b * Hn + j) * D + col] = acc;
    }
    c = cn;
  }
}

}  // namespace

static bool sue_seg_pool_ok(int B, int N, int Hn, int C, int D) {
  return B >= 1 && N >= 1 && N <= 8 && Hn >= 1 && Hn <= SUE_MAXH && C >= 1 && C <= SUE_MAXC && D >= 1;
}
extern "C" int nnr_sue_seg_pool_fwd(const float* x, const float* u, const long* cidx, int B, int N, int Hn, int C, int D, float scale,
                                    float* alpha, float* feat, hipStream_t stream) {
  if (!sue_seg_pool_ok(B, N, Hn, C, D)) return NNR_ERR_UNSUPPORTED;
  if (!x || !u || !cidx || !alpha || !feat) return NNR_ERR_ARG;
  hipLaunchKernelGGL(sue_seg_pool_fwd_kernel, dim3((B + 7) / 8 * 8 * N), dim3(256), 0, stream, x, u, cidx, B, N, Hn, C, D, scale, alpha, feat);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
extern "C" int nnr_sue_seg_pool_bwd(const float* x, const float* u, const long* cidx, const float* alpha, const float* dfeat, int B, int N,
                                    int Hn, int C, int D, float scale, float* dx, float* du, float* ds_ws, hipStream_t stream) {
  if (!sue_seg_pool_ok(B, N, Hn, C, D)) return NNR_ERR_UNSUPPORTED;
  if (!x || !u || !cidx || !alpha || !dfeat || !dx || !du || !ds_ws) return NNR_ERR_ARG;
  hipLaunchKernelGGL(sue_seg_pool_bwd_ds_kernel, dim3((B + 7) / 8 * 8 * N), dim3(256), 0, stream, x, cidx, alpha, dfeat, B, N, Hn, C, D, scale,
                     ds_ws, du);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sue_seg_pool_bwd_dx_kernel, dim3(B, (D + 255) / 256, C >= 3 ? 3 : 1), dim3(256), 0, stream, u, cidx, alpha, dfeat, ds_ws, N,
                     Hn, C, D, dx);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
