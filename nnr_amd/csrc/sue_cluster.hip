// SUE's segmented cluster attention (userEncoders.py:85-89; replaces torch_scatter.scatter_softmax / scatter_sum), in its two forms:
//   keys form  sue_intra_*     s_h = <K(g_h), q_n> / sqrt(A) on a projected key buffer kf [B Hn, A]      (SUE)
//   GEMV form  sue_seg_pool_*  s_h = scale <x_h, u_n>, u = q W_K: the key projection folded into the query  (SUE_wo_GCN, variantEncoders.py:377-381)
// Both: alpha = softmax of s WITHIN each cluster id (segments held in LDS), feat_c = sum_{h in c} alpha_h row_h -> [C, D]; empty clusters give 0.
// The limits, the work split, the cluster-id loader, the segment softmax and its backward and the three row walks are written once below; the
// kernels differ in where their scores come from and in the extra ds * u term of the GEMV form's second backward kernel.
#include "common.h"

namespace {

constexpr int SUE_MAXH = 64, SUE_MAXC = 32, SUE_MAXN = 8;

// the one size rule of the four entry points (mirrored by ops.seg_pool_supported)
bool sue_cluster_ok(int B, int N, int Hn, int C, int D) {
  return B >= 1 && N >= 1 && N <= SUE_MAXN && Hn >= 1 && Hn <= SUE_MAXH && C >= 1 && C <= SUE_MAXC && D >= 1;
}

// (nt in the helpers below: the thread stride of the caller's loops -- 256, or blockDim.x in the kernel written for any multiple of 64 threads.)
// cluster ids of user b into LDS.  Out-of-range ids are clamped into [0, C) (torch_scatter would raise; here they index cmax[] / csum[] and
// become store addresses, so they must not leave the range).
__device__ __forceinline__ void sue_load_cid(const long* __restrict__ cidx, int b, int Hn, int C, int nt, int* cid) {
  for (int j = threadIdx.x; j < Hn; j += nt) cid[j] = (int)min(max(cidx[(long)b * Hn + j], 0L), (long)(C - 1));
}

// cluster member lists of one user in LDS: order[cstart[c] .. cstart[c] + ccnt[c]) = the items of cluster c, ascending
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

// Round 6: the N candidates of a user all read the user's [Hn, D] rows (180 KB; the launch's algorithmic bytes count them ONCE), and consecutive
// workgroup ids go to different XCDs, whose L2s do not share: as a (B N, slices) grid the five readers of a slice sat in five L2s and the counter
// traffic was 2.6x the algorithmic bytes.  The grids are 1-D and workgroup id -> (XCD x = id & 7, slot = id >> 3) -> user b = 8 (slot / per_user) + x:
// every workgroup of a user runs on ONE XCD, its readers back to back.
__device__ __forceinline__ bool sue_xcd_map(int id, int B, int per_user, int* b, int* w) {
  const int x = id & 7, slot = id >> 3;
  *b = (slot / per_user) * 8 + x;
  *w = slot % per_user;
  return *b < B;
}

// al[j] = softmax of sc[] within the cluster of j (cmax / csum: one thread per cluster over its member list), also written to alpha_row if given
__device__ __forceinline__ void sue_seg_softmax(const float* sc, const int* cid, const int* order, const int* ccnt, const int* cstart, int Hn,
                                                int C, int nt, float* cmax, float* csum, float* al, float* alpha_row) {
  const int tid = threadIdx.x;
  if (tid < C) {
    float m = -INFINITY;
    for (int k = 0; k < ccnt[tid]; ++k) m = fmaxf(m, sc[order[cstart[tid] + k]]);
    float sm = 0.f;
    for (int k = 0; k < ccnt[tid]; ++k) sm += expf(sc[order[cstart[tid] + k]] - m);
    cmax[tid] = m; csum[tid] = sm;
  }
  __syncthreads();
  for (int j = tid; j < Hn; j += nt) {
    const float v = expf(sc[j] - cmax[cid[j]]) / csum[cid[j]];
    al[j] = v;
    if (alpha_row) alpha_row[j] = v;
  }
  __syncthreads();
}

// One column of the C cluster features: fo[c D] = sum_{j in c} al[j] gb[j D].  One walk over the cluster-sorted member list, 8 loads in flight per
// trip (cluster by cluster the walk was up to Hn dependent loads: clusters hold 2-3 members on average).  Every cluster sums its members in
// ascending order; an empty cluster gives exactly 0, as scatter_sum.
__device__ __forceinline__ void sue_walk_column(const float* gb, float* fo, int D, int C, const int* cid,
                                                const int* order, const int* ccnt, const int* cstart, const float* al) {
  for (int c = 0; c < C; ++c)
    if (ccnt[c] == 0) fo[(long)c * D] = 0.f;
  const int total = cstart[C - 1] + ccnt[C - 1];         // == Hn: every item sits in one cluster
  if (total == 0) return;
  int cur = cid[order[0]];
  float acc = 0.f;
  for (int p0 = 0; p0 < total; p0 += 8) {
    int jj[8];
    float gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      jj[u] = order[min(p0 + u, total - 1)];
      gv[u] = gb[(long)jj[u] * D];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (p0 + u < total) {
        const int cl = cid[jj[u]];
        if (cl != cur) {
          fo[(long)cur * D] = acc;
          acc = 0.f;
          cur = cl;
        }
        acc += al[jj[u]] * gv[u];
      }
    }
  }
  fo[(long)cur * D] = acc;
}

// out[j] = mul * <other[(ridx ? ridx[j] : 0), :], xb[j, :]> for the Hn rows of one user, by the waves of the workgroup.  Rows of float4 when D and both
// bases allow 16-byte loads (sue_rows_f4), else row by row with scalar lanes.
__device__ __forceinline__ bool sue_rows_f4(const float* xb, const float* other, int D) {
  return !(D & 3) && !((reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(other)) & 15);
}
__device__ __forceinline__ void sue_row_dots_scalar(const float* __restrict__ xb, const float* __restrict__ other, const int* ridx, int Hn, int D,
                                                    float mul, float* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int j = w; j < Hn; j += nw) {
    const float* ar = other + (ridx ? (long)ridx[j] * D : 0L);
    const float* cr = xb + (long)j * D;
    float p = 0.f;
    for (int x = lane; x < D; x += 64) p += ar[x] * cr[x];
    p = wave_sum(p);
    if (lane == 0) out[j] = p * mul;
  }
}
// 4 rows per wave and trip with float4 lanes, one column trip per pass.  (sue_intra_bwd_ds_kernel keeps a two-trip form of this loop in its body: as
// one template over the trip count the compiler contracted the multiply-adds of that kernel differently, which moved SUE's results by an ulp --
// profiles/sue_pipeline_summary.md.  Both add a lane's columns in ascending order.)
__device__ __forceinline__ void sue_row_dots(const float* __restrict__ xb, const float* __restrict__ other, const int* ridx, int Hn, int D,
                                             float mul, float* out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  if (!sue_rows_f4(xb, other, D)) return sue_row_dots_scalar(xb, other, ridx, Hn, D, mul, out);
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
}

// segment-softmax backward: ds[j] = al[j] (da[j] - sum_{i in cluster(j)} al[i] da[i]) scale, also written to the workspace row
__device__ __forceinline__ void sue_seg_softmax_bwd(const float* al, const float* da, const int* cid, int Hn, int C, int nt, float scale, float* csum,
                                                    float* ds, float* ds_ws, long row0) {
  const int tid = threadIdx.x;
  if (tid < C) {
    float sm = 0.f;
    for (int j = 0; j < Hn; ++j) if (cid[j] == tid) sm += al[j] * da[j];
    csum[tid] = sm;
  }
  __syncthreads();
  for (int j = tid; j < Hn; j += nt) {
    const float v = al[j] * (da[j] - csum[cid[j]]) * scale;
    ds[j] = v;
    ds_ws[row0 + j] = v;
  }
  __syncthreads();
}

// sum_j ds[j] rows[j ld + x], j ascending, 8 loads in flight
__device__ __forceinline__ float sue_ds_rows_sum(const float* ds, const float* rows, long ld, int Hn, int x) {
  float acc = 0.f;
  int j = 0;
  for (; j + 8 <= Hn; j += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = rows[(long)(j + u) * ld + x];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += ds[j + u] * v[u];
  }
  for (; j < Hn; ++j) acc += ds[j] * rows[(long)j * ld + x];
  return acc;
}

// One column of the history-row gradient: out[(b Hn + j) D + col] = sum_n (al[n][j] dfeat[b, n, c(j), col] (+ ds[n][j] uv[n] if WITH_U)), n ascending.
// Every row belongs to exactly one cluster and blockIdx.z deals the clusters (c = z, z + Z, ...), so each element is written exactly once (no
// read-modify-write): B * slices workgroups alone are 1.25 waves per SIMD at batch 64, and their C dependent load groups were pure latency.  The
// next cluster's d feat values are loaded before this cluster's rows are stored.  Rows n >= N of the LDS tables are never written (stale LDS may
// hold NaN) and are not read.
template <bool WITH_U>
__device__ __forceinline__ void sue_deal_clusters(const float* dfeat, int b, int N, int Hn, int C, int D, int col,
                                                  const float (*al)[SUE_MAXH], const float (*ds)[SUE_MAXH], const float* uv, const int* order,
                                                  const int* ccnt, const int* cstart, float* out) {
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
      for (int n = 0; n < 8; ++n) {
        if (n < N) {
          if (WITH_U) acc += al[n][j] * dv[n] + ds[n][j] * uv[n];
          else acc += al[n][j] * dv[n];
        }
      }
      out[((long)b * Hn + j) * D + col] = acc;
    }
    c = cn;
  }
}

// ---------------------------------------------------------------------------------------------- keys form (SUE)
// forward: one workgroup per (b, n, 256-column slice), all of a user on one XCD, the N readers of a slice back to back (n fastest) -- every
// workgroup recomputes the (tiny) scores and segment softmax of its (b, n) and produces one slice of the C cluster features.
__global__ __launch_bounds__(256) void sue_intra_fwd_kernel(const float* __restrict__ kf, const float* __restrict__ qc,
                                                            const float* __restrict__ g, const long* __restrict__ cidx,
                                                            int B, int N, int Hn, int C, int A, int D, float inv_scale,
                                                            float* __restrict__ alpha, float* __restrict__ feat) {
  __shared__ float sc[SUE_MAXH], al[SUE_MAXH], cmax[SUE_MAXC], csum[SUE_MAXC];
  __shared__ int cid[SUE_MAXH], order[SUE_MAXH], ccnt[SUE_MAXC], cstart[SUE_MAXC];
  int b, wi;
  if (!sue_xcd_map(blockIdx.x, B, N * ((D + 255) / 256), &b, &wi)) return;
  const int slice = wi / N, bn = b * N + (wi - slice * N);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  sue_load_cid(cidx, b, Hn, C, 256, cid);
  const float* q = qc + (long)bn * A;
  for (int j0 = w; j0 < Hn; j0 += 16) {                     // 4 items per wave and trip: their loads are in flight together
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    const float* k[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) k[u] = kf + ((long)b * Hn + min(j0 + 4 * u, Hn - 1)) * A;
    for (int x = lane; x < A; x += 64) {
      const float qv = q[x];
      float kv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) kv[u] = k[u][x];
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u] += kv[u] * qv;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = wave_sum(p[u]);
      if (lane == 0 && j0 + 4 * u < Hn) sc[j0 + 4 * u] = t * inv_scale;
    }
  }
  __syncthreads();
  sue_members(cid, Hn, C, ccnt, cstart, order);
  sue_seg_softmax(sc, cid, order, ccnt, cstart, Hn, C, 256, cmax, csum, al, slice == 0 ? alpha + (long)bn * Hn : nullptr);
  const int col = slice * 256 + tid;
  if (col >= D) return;
  sue_walk_column(g + (long)b * Hn * D + col, feat + (long)bn * C * D + col, D, C, cid, order, ccnt, cstart, al);
}

// backward part 1, grid B*N: dalpha_j = <dfeat[cid_j], g_j>, segment-softmax backward -> ds[b, n, :] (workspace), dqc[b, n, :] = sum_j ds[j] kf[b, j, :].
// (B*N = 320 workgroups of 4 waves at batch 64.  16 waves per workgroup take the Hn items in one trip and are no faster alone
// (30 vs 27 us) but 126 vs 82 us inside the step: a 1024-thread workgroup needs a whole CU at once, and the CUs are shared with the
// weight-gradient GEMM of the other stream.  The kernel is written for any multiple of 64 threads.)
__global__ __launch_bounds__(256) void sue_intra_bwd_ds_kernel(const float* __restrict__ kf, const float* __restrict__ g,
                                                                const long* __restrict__ cidx, const float* __restrict__ alpha,
                                                                const float* __restrict__ dfeat, int B, int N, int Hn, int C, int A, int D,
                                                                float inv_scale, float* __restrict__ ds_ws, float* __restrict__ dqc) {
  __shared__ float al[SUE_MAXH], da[SUE_MAXH], ds[SUE_MAXH], csum[SUE_MAXC];
  __shared__ int cid[SUE_MAXH];
  int b, ni;
  if (!sue_xcd_map(blockIdx.x, B, N, &b, &ni)) return;             // (the N workgroups of a user read the same g[b]: one XCD, see the forward)
  const int bn = b * N + ni, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  sue_load_cid(cidx, b, Hn, C, nt, cid);
  for (int j = tid; j < Hn; j += nt) al[j] = alpha[(long)bn * Hn + j];
  __syncthreads();
  const float* gb = g + (long)b * Hn * D;
  const float* df = dfeat + (long)bn * C * D;
  // dalpha_j = <dfeat[cid_j], g_j>
  if (sue_rows_f4(gb, df, D)) {
    // 4 items per wave at a time, float4 lanes, two column trips per pass: 16 independent 16-byte loads in flight, 2 passes at D = 900
    const int D4 = D >> 2;
    for (int j0 = w; j0 < Hn; j0 += 4 * nw) {
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      const f32x4* dr[4];
      const f32x4* gr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = min(j0 + nw * u, Hn - 1);
        dr[u] = reinterpret_cast<const f32x4*>(df + (long)cid[j] * D);
        gr[u] = reinterpret_cast<const f32x4*>(gb + (long)j * D);
      }
      for (int x = lane; x < D4; x += 128) {
        const int x2 = x + 64;
        const bool two = x2 < D4;
        f32x4 a[4], c[4], a2[4], c2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = dr[u][x]; c[u] = gr[u][x]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a2[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          c2[u] = a2[u];
          if (two) { a2[u] = dr[u][x2]; c2[u] = gr[u][x2]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] += a[u][0] * c[u][0] + a[u][1] * c[u][1] + a[u][2] * c[u][2] + a[u][3] * c[u][3];
        if (two) {
#pragma unroll
          for (int u = 0; u < 4; ++u) p[u] += a2[u][0] * c2[u][0] + a2[u][1] * c2[u][1] + a2[u][2] * c2[u][2] + a2[u][3] * c2[u][3];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float t = wave_sum(p[u]);
        if (lane == 0 && j0 + nw * u < Hn) da[j0 + nw * u] = t;
      }
    }
  } else {
    sue_row_dots_scalar(gb, df, cid, Hn, D, 1.f, da);
  }
  __syncthreads();
  sue_seg_softmax_bwd(al, da, cid, Hn, C, nt, inv_scale, csum, ds, ds_ws, (long)bn * Hn);
  for (int x = tid; x < A; x += nt) dqc[(long)bn * A + x] = sue_ds_rows_sum(ds, kf + (long)b * Hn * A, A, Hn, x);
}

// backward part 2, grid (B, ceil(D/256) + 1, Z): slices y < last -> dg[b, j, cols] = sum_n alpha[b,n,j] * dfeat[b,n,cid_j,cols];
// the last slice -> dkf[b, j, :] = sum_n ds[b,n,j] * qc[b,n,:]
__global__ __launch_bounds__(256) void sue_intra_bwd_dg_kernel(const float* __restrict__ qc, const long* __restrict__ cidx,
                                                               const float* __restrict__ alpha, const float* __restrict__ dfeat,
                                                               const float* __restrict__ ds_ws, int N, int Hn, int C, int A, int D,
                                                               float* __restrict__ dg, float* __restrict__ dkf) {
  __shared__ float al[8][SUE_MAXH];
  __shared__ int cid[SUE_MAXH], order[SUE_MAXH], ccnt[SUE_MAXC], cstart[SUE_MAXC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool last = blockIdx.y == gridDim.y - 1;
  for (int i = tid; i < N * Hn; i += 256) {
    const int n = i / Hn, j = i - n * Hn;
    al[n][j] = last ? ds_ws[((long)b * N + n) * Hn + j] : alpha[((long)b * N + n) * Hn + j];
  }
  sue_load_cid(cidx, b, Hn, C, 256, cid);
  __syncthreads();
  if (last) {
    if (blockIdx.z) return;
    for (int x = tid; x < A; x += 256) {
      float qv[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) qv[n] = n < N ? qc[((long)b * N + n) * A + x] : 0.f;
      for (int j = 0; j < Hn; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) if (n < N) acc += al[n][j] * qv[n];      // rows n >= N of `al` are never written (stale LDS may hold NaN)
        dkf[((long)b * Hn + j) * A + x] = acc;
      }
    }
    return;
  }
  sue_members(cid, Hn, C, ccnt, cstart, order);
  const int col = blockIdx.y * 256 + tid;
  if (col >= D) return;
  sue_deal_clusters<false>(dfeat, b, N, Hn, C, D, col, al, nullptr, nullptr, order, ccnt, cstart, dg);
}

// ---------------------------------------------------------------------------------------------- GEMV form (SUE_wo_GCN)
// The key projection's bias adds one constant to every score of a (user, candidate) and cancels in each segment softmax, so
// K(x_h) . q_n = x_h . (W_K^T q_n) = x_h . u_n  and the [B Hn, A] key buffer never exists.
// forward: one workgroup per (b, n), the N workgroups of a user on one XCD: scores over D, segment softmax, then every thread walks the
// cluster-sorted member list once per column it owns.
__global__ __launch_bounds__(256) void sue_seg_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                                const long* __restrict__ cidx, int B, int N, int Hn, int C, int D, float scale,
                                                                float* __restrict__ alpha, float* __restrict__ feat) {
  __shared__ float sc[SUE_MAXH], al[SUE_MAXH], cmax[SUE_MAXC], csum[SUE_MAXC];
  __shared__ int cid[SUE_MAXH], order[SUE_MAXH], ccnt[SUE_MAXC], cstart[SUE_MAXC];
  int b, ni;
  if (!sue_xcd_map(blockIdx.x, B, N, &b, &ni)) return;
  const int bn = b * N + ni, tid = threadIdx.x;
  sue_load_cid(cidx, b, Hn, C, 256, cid);
  const float* xb = x + (long)b * Hn * D;
  sue_row_dots(xb, u + (long)bn * D, nullptr, Hn, D, scale, sc);
  __syncthreads();
  sue_members(cid, Hn, C, ccnt, cstart, order);
  sue_seg_softmax(sc, cid, order, ccnt, cstart, Hn, C, 256, cmax, csum, al, alpha + (long)bn * Hn);
  for (int col = tid; col < D; col += 256)
    sue_walk_column(xb + col, feat + (long)bn * C * D + col, D, C, cid, order, ccnt, cstart, al);
}

// backward part 1, one workgroup per (b, n): dalpha_h = <dfeat[c(h)], x_h>, the segment-softmax backward -> ds[b, n, :] (scaled; workspace)
// and du[b, n, :] = sum_h ds_h x_h, h ascending.  Five waves per SIMD is what this body has always run at, two registers below the limit of 96;
// the bound says so, since the allocation moves by that much with the code around the kernel.
__global__ __launch_bounds__(256, 5) void sue_seg_pool_bwd_ds_kernel(const float* __restrict__ x, const long* __restrict__ cidx,
                                                                   const float* __restrict__ alpha, const float* __restrict__ dfeat, int B,
                                                                   int N, int Hn, int C, int D, float scale, float* __restrict__ ds_ws,
                                                                   float* __restrict__ du) {
  __shared__ float al[SUE_MAXH], da[SUE_MAXH], ds[SUE_MAXH], csum[SUE_MAXC];
  __shared__ int cid[SUE_MAXH];
  int b, ni;
  if (!sue_xcd_map(blockIdx.x, B, N, &b, &ni)) return;
  const int bn = b * N + ni, tid = threadIdx.x;
  sue_load_cid(cidx, b, Hn, C, 256, cid);
  for (int j = tid; j < Hn; j += 256) al[j] = alpha[(long)bn * Hn + j];
  __syncthreads();
  const float* xb = x + (long)b * Hn * D;
  sue_row_dots(xb, dfeat + (long)bn * C * D, cid, Hn, D, 1.f, da);
  __syncthreads();
  sue_seg_softmax_bwd(al, da, cid, Hn, C, 256, scale, csum, ds, ds_ws, (long)bn * Hn);
  for (int col = tid; col < D; col += 256) du[(long)bn * D + col] = sue_ds_rows_sum(ds, xb, D, Hn, col);
}

// backward part 2, grid (B, ceil(D/256), Z): dx[b, h, cols] = sum_n (alpha[b,n,h] dfeat[b,n,c(h),cols] + ds[b,n,h] u[b,n,cols]), n ascending
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
  sue_load_cid(cidx, b, Hn, C, 256, cid);
  __syncthreads();
  sue_members(cid, Hn, C, ccnt, cstart, order);
  const int col = blockIdx.y * 256 + tid;
  if (col >= D) return;
  float uv[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) uv[n] = n < N ? u[((long)b * N + n) * D + col] : 0.f;
  sue_deal_clusters<true>(dfeat, b, N, Hn, C, D, col, al, ds, uv, order, ccnt, cstart, dx);
}

}  // namespace

extern "C" int nnr_sue_intra_fwd(const float* kf, const float* qc, const float* g, const long* cidx, int B, int N, int Hn, int C, int A,
                                 int D, float* alpha, float* feat, hipStream_t stream) {
  if (!sue_cluster_ok(B, N, Hn, C, D) || A < 1) return NNR_ERR_UNSUPPORTED;
  if (!kf || !qc || !g || !cidx || !alpha || !feat) return NNR_ERR_ARG;
  hipLaunchKernelGGL(sue_intra_fwd_kernel, dim3((B + 7) / 8 * 8 * N * ((D + 255) / 256)), dim3(256), 0, stream, kf, qc, g, cidx, B, N, Hn, C, A, D,
                     1.f / sqrtf((float)A), alpha, feat);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
extern "C" int nnr_sue_intra_bwd(const float* kf, const float* qc, const float* g, const long* cidx, const float* alpha,
                                 const float* dfeat, int B, int N, int Hn, int C, int A, int D, float* dg, float* dkf, float* dqc,
                                 float* ds_ws, hipStream_t stream) {
  if (!sue_cluster_ok(B, N, Hn, C, D) || A < 1) return NNR_ERR_UNSUPPORTED;
  if (!kf || !qc || !g || !cidx || !alpha || !dfeat || !dg || !dkf || !dqc || !ds_ws) return NNR_ERR_ARG;
  hipLaunchKernelGGL(sue_intra_bwd_ds_kernel, dim3((B + 7) / 8 * 8 * N), dim3(256), 0, stream, kf, g, cidx, alpha, dfeat, B, N, Hn, C, A, D,
                     1.f / sqrtf((float)A), ds_ws, dqc);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sue_intra_bwd_dg_kernel, dim3(B, (D + 255) / 256 + 1, C >= 3 ? 3 : 1), dim3(256), 0, stream, qc, cidx, alpha, dfeat, ds_ws, N, Hn, C,
                     A, D, dg, dkf);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
extern "C" int nnr_sue_seg_pool_fwd(const float* x, const float* u, const long* cidx, int B, int N, int Hn, int C, int D, float scale,
                                    float* alpha, float* feat, hipStream_t stream) {
  if (!sue_cluster_ok(B, N, Hn, C, D)) return NNR_ERR_UNSUPPORTED;
  if (!x || !u || !cidx || !alpha || !feat) return NNR_ERR_ARG;
  hipLaunchKernelGGL(sue_seg_pool_fwd_kernel, dim3((B + 7) / 8 * 8 * N), dim3(256), 0, stream, x, u, cidx, B, N, Hn, C, D, scale, alpha, feat);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
extern "C" int nnr_sue_seg_pool_bwd(const float* x, const float* u, const long* cidx, const float* alpha, const float* dfeat, int B, int N,
                                    int Hn, int C, int D, float scale, float* dx, float* du, float* ds_ws, hipStream_t stream) {
  if (!sue_cluster_ok(B, N, Hn, C, D)) return NNR_ERR_UNSUPPORTED;
  if (!x || !u || !cidx || !alpha || !dfeat || !dx || !du || !ds_ws) return NNR_ERR_ARG;
  hipLaunchKernelGGL(sue_seg_pool_bwd_ds_kernel, dim3((B + 7) / 8 * 8 * N), dim3(256), 0, stream, x, cidx, alpha, dfeat, B, N, Hn, C, D, scale,
                     ds_ws, du);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sue_seg_pool_bwd_dx_kernel, dim3(B, (D + 255) / 256, C >= 3 ? 3 : 1), dim3(256), 0, stream, u, cidx, alpha, dfeat, ds_ws, N, Hn, C,
                     D, dx);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
