// Masked-softmax attention pooling, one workgroup (4 waves) per sequence / group; wave-shuffle softmax.
// Replaces the softmax + bmm(alpha, feature) tails of `Attention` (layers.py:169-175) and
// `ScaledDotProduct_CandidateAttention` (layers.py:197-203) and their backward.
//
//   layout PACKED : item (s, t) lives at row off[t] + s of x (time-major packed, see seq_plan.hip), t < slen[s];
//                   outputs / query vectors are indexed by order[s] (the caller's news order).
//   layout DENSE  : item (s, t) lives at row s*L + t, optional mask[(s / mask_div)*L + t] (0 -> score = -1e9, exactly
//                   as masked_fill(mask == 0, -1e9) in the reference); outputs indexed by s.
//   score GIVEN   : score[row] precomputed (additive attention: w2 . tanh(W1 x + b1), fused into the GEMM epilogue).
//   score DOT     : score = scale * <x[row], v[oidx]>   with v = K^T (Q q + b_Q)  -- the algebraic form of
//                   (K x).(Q q) that turns the [tokens, F] x [F, A] projection of every token into one GEMV per news.
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int MAXT = 2;   // positions per lane: supports L <= 128 (the selects below assume exactly 2)
constexpr int MAXV_ALL = 5;   // float4 per lane:   supports D <= 1280 (SUE at --hidden_dim 256: D = 1124)

struct PoolArgs {
  const float* x; int ldx; int D; int n; int L;
  int packed;
  const int* off; const int* slen; const int* order;
  const uint8_t* mask; int mask_div;
  const float* score;            // GIVEN
  const float* v; int ldv; float scale;   // DOT
  float* alpha;                  // [rows] (PACKED: packed row; DENSE: s*L+t)
  float* out; int ldo; const float* add_in; int ldadd;
  // backward
  const float* dout; int lddo; const float* dout2; int lddo2;
  float* dx; int lddx; int dx_accumulate;
  float* dscore;
  float* dv; int lddv;
  const float* th; int ldth; int A; const float* w2;      // score = <th[row, :A], w2> computed here (forward)
  // backward: a second pool's token gradient folded into the one write of dx (see nnr_pool_args)
  const float* alpha_b; const float* dout_b; int lddo_b; const float* dscore_b; const float* v_b; int ldv_b; float scale_b;
};

__device__ __forceinline__ long item_row(const PoolArgs& a, int s, int t) {
  return a.packed ? (long)a.off[t] + s : (long)s * a.L + t;
}

// One WORKGROUP (4 waves) per sequence: wave w owns the token chunks c = w, w+4, ... (UR tokens each), so a 128-token abstract
// is 8 dependent iterations per pass instead of 32 (one wave per sequence measured 70 / 187 us fwd / bwd on the history call,
// a quarter of the HBM rate, bound by that serial walk).  Per-token scalars (scores, d alpha) meet in LDS and the softmax is
// recomputed by every wave (L <= 128 values); partial D-vectors (weighted sum, d v) are reduced across the waves through LDS.
template <bool BWD, int NV, int UR>
__device__ __forceinline__ void pool_stream_body(const PoolArgs& a, const int s, float* __restrict__ tok, f32x4 (*__restrict__ part)[64 * NV]) {
  constexpr int MAXV = NV;     // float4 per lane actually needed for this D (shadows the file-level bound)
  constexpr int NWV = 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (s >= a.n) return;
  const int len = a.packed ? a.slen[s] : a.L;
  const int oidx = a.packed ? a.order[s] : s;
  const int nv = (a.D + 3) >> 2;           // float4 per row (D % 4 == 0 required)
  const bool dot = a.v != nullptr;

  f32x4 q[MAXV];                           // DOT: query vector v
  if (dot) {
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      const int c = lane + 64 * j;
      q[j] = (c < nv) ? *reinterpret_cast<const f32x4*>(a.v + (long)oidx * a.ldv + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  // UR rows in flight per iteration: the row loads are independent, only the shuffle reductions are serial
  auto load_rows = [&](int t0, f32x4 (&xv)[UR][MAXV]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int t = min(t0 + u, len - 1);
      const float* xr = a.x + item_row(a, s, t) * a.ldx;
#pragma unroll
      for (int j = 0; j < MAXV; ++j) {
        const int c = lane + 64 * j;
        xv[u][j] = (c < nv) ? *reinterpret_cast<const f32x4*>(xr + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  // sum of the 4 waves' partial vectors -> every wave gets the total
  auto reduce_vec = [&](f32x4 (&v)[MAXV]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < MAXV; ++j) part[w][lane + 64 * j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MAXV; ++j) v[j] = part[0][lane + 64 * j] + part[1][lane + 64 * j] + part[2][lane + 64 * j] + part[3][lane + 64 * j];
  };

  if (!BWD) {
    // ---- scores
    float sc[MAXT];
    if (dot) {
      for (int t0 = w * UR; t0 < len; t0 += NWV * UR) {
        f32x4 xv[UR][MAXV];
        load_rows(t0, xv);
#pragma unroll
        for (int u = 0; u < UR; ++u) {
          const int t = t0 + u;
          float p = 0.f;
#pragma unroll
          for (int j = 0; j < MAXV; ++j) p += xv[u][j][0] * q[j][0] + xv[u][j][1] * q[j][1] + xv[u][j][2] * q[j][2] + xv[u][j][3] * q[j][3];
          p = wave_sum(p) * a.scale;
          if (t < len && lane == 0) tok[t] = p;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < MAXT; ++k) {
        const int t = lane + 64 * k;
        sc[k] = (t < len) ? tok[t] : -INFINITY;
      }
    } else if (a.th) {
      // additive-attention score w2 . tanh(W1 x + b1) from the tanh rows: wave w takes tokens w, w + 4, ... (4 rows in flight)
      const int na = a.A >> 2;
      const f32x4 wv = (lane < na) ? *reinterpret_cast<const f32x4*>(a.w2 + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
      for (int t0 = w; t0 < len; t0 += 4 * NWV) {
        f32x4 tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = min(t0 + u * NWV, len - 1);
          tv[u] = (lane < na) ? *reinterpret_cast<const f32x4*>(a.th + item_row(a, s, t) * a.ldth + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + u * NWV;
          float p = tv[u][0] * wv[0] + tv[u][1] * wv[1] + tv[u][2] * wv[2] + tv[u][3] * wv[3];
          p = wave_sum(p);
          if (t < len && lane == 0) tok[t] = p;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < MAXT; ++k) {
        const int t = lane + 64 * k;
        sc[k] = (t < len) ? tok[t] : -INFINITY;
      }
    } else {
#pragma unroll
      for (int k = 0; k < MAXT; ++k) {
        const int t = lane + 64 * k;
        sc[k] = (t < len) ? a.score[item_row(a, s, t)] : -INFINITY;
      }
    }
    if (a.mask) {
#pragma unroll
      for (int k = 0; k < MAXT; ++k) {
        const int t = lane + 64 * k;
        if (t < len && !a.mask[(long)((a.packed ? oidx : s) / a.mask_div) * a.L + t]) sc[k] = -1e9f;      // (packed: the mask is in the caller's row order)
      }
    }
    // ---- softmax over t < len (every wave computes the same values)
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) m = fmaxf(m, sc[k]);
    m = wave_max(m);
    float e[MAXT], sum = 0.f;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      const int t = lane + 64 * k;
      e[k] = (t < len) ? expf(sc[k] - m) : 0.f;
      sum += e[k];
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      const int t = lane + 64 * k;
      e[k] *= inv;
      if (w == 0 && t < len && a.alpha) a.alpha[item_row(a, s, t)] = e[k];
    }
    // ---- weighted sum
    f32x4 acc[MAXV];
#pragma unroll
    for (int j = 0; j < MAXV; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t0 = w * UR; t0 < len; t0 += NWV * UR) {
      f32x4 xv[UR][MAXV];
      load_rows(t0, xv);
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int t = t0 + u;
        const float al = (t < len) ? __shfl(t < 64 ? e[0] : e[1], t & 63, 64) : 0.f;
#pragma unroll
        for (int j = 0; j < MAXV; ++j) acc[j] += al * xv[u][j];
      }
    }
    reduce_vec(acc);
    if (w == 0) {
#pragma unroll
      for (int j = 0; j < MAXV; ++j) {
        const int c = lane + 64 * j;
        if (c < nv) {
          f32x4 o = acc[j];
          if (a.add_in) o += *reinterpret_cast<const f32x4*>(a.add_in + (long)oidx * a.ldadd + 4 * c);
          *reinterpret_cast<f32x4*>(a.out + (long)oidx * a.ldo + 4 * c) = o;
        }
      }
    }
  } else {
    // ---------------------------------------------------------------- backward
    f32x4 go[MAXV];
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      const int c = lane + 64 * j;
      go[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < nv) {
        go[j] = *reinterpret_cast<const f32x4*>(a.dout + (long)oidx * a.lddo + 4 * c);
        if (a.dout2) go[j] += *reinterpret_cast<const f32x4*>(a.dout2 + (long)oidx * a.lddo2 + 4 * c);
      }
    }
    float al[MAXT], da[MAXT];
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      const int t = lane + 64 * k;
      al[k] = (t < len) ? a.alpha[item_row(a, s, t)] : 0.f;
    }
    // dalpha_t = <dout, x_t>
    for (int t0 = w * UR; t0 < len; t0 += NWV * UR) {
      f32x4 xv[UR][MAXV];
      load_rows(t0, xv);
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int t = t0 + u;
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < MAXV; ++j) p += xv[u][j][0] * go[j][0] + xv[u][j][1] * go[j][1] + xv[u][j][2] * go[j][2] + xv[u][j][3] * go[j][3];
        p = wave_sum(p);
        if (t < len && lane == 0) tok[t] = p;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      const int t = lane + 64 * k;
      da[k] = (t < len) ? tok[t] : 0.f;
    }
    float dsum = 0.f;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) dsum += al[k] * da[k];
    dsum = wave_sum(dsum);
    float ds[MAXT];
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      const int t = lane + 64 * k;
      ds[k] = al[k] * (da[k] - dsum);          // d loss / d score_t (masked items have alpha = 0 -> 0)
      // ... except in a FULLY masked group (every score is the constant -1e9: alpha is uniform, not 0): masked_fill passes no gradient
      // to the score it replaced (layers.py:171,199)
      if (a.mask && t < len && !a.mask[(long)((a.packed ? oidx : s) / a.mask_div) * a.L + t]) ds[k] = 0.f;
      if (w == 0 && t < len && a.dscore) a.dscore[item_row(a, s, t)] = ds[k];
    }
    f32x4 dvacc[MAXV];
#pragma unroll
    for (int j = 0; j < MAXV; ++j) dvacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!a.dx && !(dot && a.dv)) return;        // nothing but dscore was wanted
    // the second pool's terms (alpha_b * dout_b + scale_b * dscore_b * v_b): per-sequence vectors and per-token scalars
    const bool two = a.alpha_b != nullptr;
    f32x4 go2[MAXV], q2[MAXV];
    float al2[MAXT], ds2[MAXT];
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      const int c = lane + 64 * j;
      go2[j] = q2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (two && c < nv) {
        go2[j] = *reinterpret_cast<const f32x4*>(a.dout_b + (long)oidx * a.lddo_b + 4 * c);
        q2[j] = *reinterpret_cast<const f32x4*>(a.v_b + (long)oidx * a.ldv_b + 4 * c);
      }
    }
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      const int t = lane + 64 * k;
      al2[k] = (two && t < len) ? a.alpha_b[item_row(a, s, t)] : 0.f;
      ds2[k] = (two && t < len) ? a.dscore_b[item_row(a, s, t)] * a.scale_b : 0.f;
    }
    for (int t0 = w * UR; t0 < len; t0 += NWV * UR) {
      f32x4 xv[UR][MAXV], old[UR][MAXV];
      long rows[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int t = min(t0 + u, len - 1);
        rows[u] = item_row(a, s, t);
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {
          const int c = lane + 64 * j;
          xv[u][j] = (dot && c < nv) ? *reinterpret_cast<const f32x4*>(a.x + rows[u] * a.ldx + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
          old[u][j] = (a.dx && a.dx_accumulate && c < nv) ? *reinterpret_cast<const f32x4*>(a.dx + rows[u] * a.lddx + 4 * c)
                                                          : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int t = t0 + u;
        if (t >= len) continue;
        const float alt = __shfl(t < 64 ? al[0] : al[1], t & 63, 64);
        const float dst = __shfl(t < 64 ? ds[0] : ds[1], t & 63, 64) * a.scale;
        const float alt2 = __shfl(t < 64 ? al2[0] : al2[1], t & 63, 64);
        const float dst2 = __shfl(t < 64 ? ds2[0] : ds2[1], t & 63, 64);
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {
          const int c = lane + 64 * j;
          if (c < nv) {
            // (two: in the association the two-pass form used -- (alpha_b dout_b + dscore_b v_b) first, as the stored `old`)
            const f32x4 prev = two ? (alt2 * go2[j] + dst2 * q2[j]) : old[u][j];
            f32x4 g = alt * go[j] + prev;
            if (dot) {
              g += dst * q[j];
              dvacc[j] += dst * xv[u][j];
            }
            if (a.dx) *reinterpret_cast<f32x4*>(a.dx + rows[u] * a.lddx + 4 * c) = g;
          }
        }
      }
    }
    if (dot && a.dv) {
      reduce_vec(dvacc);
      if (w == 0) {
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {
          const int c = lane + 64 * j;
          if (c < nv) *reinterpret_cast<f32x4*>(a.dv + (long)oidx * a.lddv + 4 * c) = dvacc[j];
        }
      }
    }
  }
}

template <bool BWD, int NV, int UR>
__global__ __launch_bounds__(256) void pool_kernel(PoolArgs a) {
  __shared__ float tok[64 * MAXT];                       // per-token scalars of the sequence (scores / d alpha)
  __shared__ f32x4 part[4][64 * NV];                     // per-wave partial vectors
  pool_stream_body<BWD, NV, UR>(a, blockIdx.x, tok, part);
}

// ------------------------------------------------------------------------------------------------ packed token streams: rows held in registers
// Round 6 (verdict item 2).  pool_stream_body walks a sequence's rows TWICE (scores, then the weighted sum; d alpha, then d x / d v) with four
// rows in flight per wave, one 4-wave workgroup per sequence whatever its length: 3 520 workgroups per launch, each a chain of 4-6 dependent
// memory round trips with a barrier between the passes, three of them resident per CU (146 VGPRs) -- 1.8 TB/s alone, 0.8 TB/s inside the step.
// A MIND-shaped batch is mostly SHORT sequences (titles: ~10 tokens), and in the time-major packed layout the rows of neighbouring sorted
// sequences at one time step are neighbours in memory.  Here a TEAM of NW waves owns a sequence and keeps its rows in registers (R = 16 rows
// of NV float4 per wave) -- every row is read ONCE, all of a wave's row loads are issued back to back (16 in flight), and both passes run out
// of registers:
//   * sequences of <= 16 tokens (sorted last: positions >= bs[16] = off[17] - off[16]): ONE WAVE each, four sequences per workgroup, no LDS,
//     no barrier -- per-token scalars are wave-uniform registers;
//   * 17 .. 64 tokens: the four waves of a workgroup share the sequence (wave w owns tokens w, w + 4, ...), scalars and partial vectors
//     meet in LDS as before;
//   * > 64 tokens (positions < bs[64]): pool_stream_body (32 rows per wave do not fit the register file).
// Workgroup b serves sequence b while b < bs[16], then sequences bs[16] + 4 (b - bs[16]) + wave; the grid stays n workgroups (the lengths
// live in device memory), the surplus exits at once.
__device__ __forceinline__ float lane_get(float v, int i) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i)); }

// Per-token scalars of a wave's R tokens live in ONE register each, token i in lane i (scores, alpha, d alpha, d score: element-wise
// arithmetic on them is one instruction for all 16 tokens, a store is one instruction; a token's value comes back as a wave-uniform
// scalar by v_readlane when a row is scaled by it).
template <bool BWD, int NV, int NW, int R>
__device__ __forceinline__ void pool_team_body(const PoolArgs& a, const int s, const int wt, float* __restrict__ tok, f32x4 (*__restrict__ part)[64 * NV]) {
  const int lane = threadIdx.x & 63;
  const int len = a.slen[s];
  const int oidx = a.order[s];
  const int nv = (a.D + 3) >> 2;
  const bool dot = a.v != nullptr;
  const long mrow = (long)(oidx / a.mask_div) * a.L;      // (packed: the mask is in the caller's row order)
  // lane i < R owns token tl = wt + NW i of the sequence; its packed row is off[tl] + s (off[] has L + 1 entries: the clamp keeps the index
  // legal, `livel` decides)
  const int tl = wt + NW * lane;
  const bool livel = lane < R && tl < len;
  const int rowl = a.off[min(tl, a.L)] + s;
  f32x4 x[R][NV];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const bool live = wt + NW * i < len;
    const long row = __builtin_amdgcn_readlane(rowl, i);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = lane + 64 * j;
      x[i][j] = (live && c < nv) ? *reinterpret_cast<const f32x4*>(a.x + row * a.ldx + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  f32x4 q[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = lane + 64 * j;
    q[j] = (dot && c < nv) ? *reinterpret_cast<const f32x4*>(a.v + (long)oidx * a.ldv + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto dotq = [&](const f32x4 (&xi)[NV], const f32x4 (&y)[NV]) __attribute__((always_inline)) {
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) p += xi[j][0] * y[j][0] + xi[j][1] * y[j][1] + xi[j][2] * y[j][2] + xi[j][3] * y[j][3];
    return wave_sum(p);
  };
  // every wave of the team gets the sum of the team's partial vectors (NW == 1: nothing to do)
  auto reduce_vec = [&](f32x4 (&v)[NV]) __attribute__((always_inline)) {
    if constexpr (NW > 1) {
#pragma unroll
      for (int j = 0; j < NV; ++j) part[wt][lane + 64 * j] = v[j];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NV; ++j) v[j] = part[0][lane + 64 * j] + part[1][lane + 64 * j] + part[2][lane + 64 * j] + part[3][lane + 64 * j];
    }
  };

  if constexpr (!BWD) {
    // ---- scores of this wave's tokens
    float pv = 0.f;
    if (dot) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const float d = dotq(x[i], q) * a.scale;
        pv = (lane == i) ? d : pv;
      }
    } else if (a.th) {
      const int na = a.A >> 2;
      const f32x4 wv = (lane < na) ? *reinterpret_cast<const f32x4*>(a.w2 + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 tv[R];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const long row = __builtin_amdgcn_readlane(rowl, i);
        tv[i] = (wt + NW * i < len && lane < na) ? *reinterpret_cast<const f32x4*>(a.th + row * a.ldth + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const float d = wave_sum(tv[i][0] * wv[0] + tv[i][1] * wv[1] + tv[i][2] * wv[2] + tv[i][3] * wv[3]);
        pv = (lane == i) ? d : pv;
      }
    } else {
      pv = livel ? a.score[rowl] : 0.f;
    }
    if (a.mask && livel && !a.mask[mrow + tl]) pv = -1e9f;
    // ---- softmax over the sequence; alv: alpha of this wave's tokens, token i in lane i
    float alv;
    if constexpr (NW == 1) {
      const float m = wave_max(livel ? pv : -INFINITY);
      const float e = livel ? expf(pv - m) : 0.f;
      alv = e * (1.f / wave_sum(e));
    } else {
      if (livel) tok[tl] = pv;
      __syncthreads();
      const float sc = (lane < len) ? tok[lane] : -INFINITY;          // (len <= 4 R <= 64 on this path: position t in lane t)
      const float m = wave_max(sc);
      float e = (lane < len) ? expf(sc - m) : 0.f;
      e *= 1.f / wave_sum(e);
      alv = __shfl(e, tl & 63, 64);
      alv = livel ? alv : 0.f;
    }
    if (a.alpha && livel) a.alpha[rowl] = alv;
    // ---- weighted sum out of the registers
    f32x4 acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float al = lane_get(alv, i);                            // (0 for a row that does not exist, whose x is 0 too)
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += al * x[i][j];
    }
    reduce_vec(acc);
    if (wt == 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int c = lane + 64 * j;
        if (c < nv) {
          f32x4 o = acc[j];
          if (a.add_in) o += *reinterpret_cast<const f32x4*>(a.add_in + (long)oidx * a.ldadd + 4 * c);
          *reinterpret_cast<f32x4*>(a.out + (long)oidx * a.ldo + 4 * c) = o;
        }
      }
    }
  } else {
    // ---------------------------------------------------------------- backward
    f32x4 go[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = lane + 64 * j;
      go[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < nv) {
        go[j] = *reinterpret_cast<const f32x4*>(a.dout + (long)oidx * a.lddo + 4 * c);
        if (a.dout2) go[j] += *reinterpret_cast<const f32x4*>(a.dout2 + (long)oidx * a.lddo2 + 4 * c);
      }
    }
    const float alv = livel ? a.alpha[rowl] : 0.f;
    float dav = 0.f;                                                // d alpha_t = <dout, x_t>
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float d = dotq(x[i], go);
      dav = (lane == i) ? d : dav;
    }
    float dsum = wave_sum(alv * dav);                               // sum_t alpha_t d alpha_t over this wave's tokens ...
    if constexpr (NW > 1) {                                         // ... and over the team
      if (lane == 0) tok[wt] = dsum;
      __syncthreads();
      dsum = (tok[0] + tok[1]) + (tok[2] + tok[3]);
    }
    float dsv = alv * (dav - dsum);              // d loss / d score_t (masked items have alpha = 0 -> 0)
    // ... except in a FULLY masked group (alpha uniform, not 0): masked_fill passes no gradient to the score it replaced (layers.py:171,199)
    if (a.mask && livel && !a.mask[mrow + tl]) dsv = 0.f;
    if (a.dscore && livel) a.dscore[rowl] = dsv;
    if (!a.dx && !(dot && a.dv)) return;        // nothing but dscore was wanted
    const bool two = a.alpha_b != nullptr;
    f32x4 go2[NV], q2[NV], dvacc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = lane + 64 * j;
      go2[j] = q2[j] = dvacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (two && c < nv) {
        go2[j] = *reinterpret_cast<const f32x4*>(a.dout_b + (long)oidx * a.lddo_b + 4 * c);
        q2[j] = *reinterpret_cast<const f32x4*>(a.v_b + (long)oidx * a.ldv_b + 4 * c);
      }
    }
    const float al2v = (two && livel) ? a.alpha_b[rowl] : 0.f;
    const float ds2v = (two && livel) ? a.dscore_b[rowl] * a.scale_b : 0.f;
    const float dstv = dsv * a.scale;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (wt + NW * i >= len) continue;
      const long row = __builtin_amdgcn_readlane(rowl, i);
      const float al = lane_get(alv, i), dst = lane_get(dstv, i), al2 = lane_get(al2v, i), ds2 = lane_get(ds2v, i);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int c = lane + 64 * j;
        if (c < nv) {
          // (two: in the association the two-pass form used -- (alpha_b dout_b + dscore_b v_b) first, as the stored `old`)
          f32x4 prev = f32x4{0.f, 0.f, 0.f, 0.f};
          if (two) prev = al2 * go2[j] + ds2 * q2[j];
          else if (a.dx && a.dx_accumulate) prev = *reinterpret_cast<const f32x4*>(a.dx + row * a.lddx + 4 * c);
          f32x4 g = al * go[j] + prev;
          if (dot) {
            g += dst * q[j];
            dvacc[j] += dst * x[i][j];
          }
          if (a.dx) *reinterpret_cast<f32x4*>(a.dx + row * a.lddx + 4 * c) = g;
        }
      }
    }
    if (dot && a.dv) {
      reduce_vec(dvacc);
      if (wt == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int c = lane + 64 * j;
          if (c < nv) *reinterpret_cast<f32x4*>(a.dv + (long)oidx * a.lddv + 4 * c) = dvacc[j];
        }
      }
    }
  }
}

template <bool BWD, int NV, int R>
__global__ __launch_bounds__(256, (R >= 16 ? 2 : 3)) void pool_packed_kernel(PoolArgs a) {
  __shared__ float tok[64 * MAXT];
  __shared__ f32x4 part[4][64 * NV];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x;
  const int nstream = a.L > 4 * R ? a.off[4 * R + 1] - a.off[4 * R] : 0;       // sequences longer than 4 R tokens (sorted first)
  const int ncoop = a.L > R ? a.off[R + 1] - a.off[R] : 0;                     // ... longer than R
  if (b < nstream) {
    pool_stream_body<BWD, NV, 4>(a, b, tok, part);
  } else if (b < ncoop) {
    pool_team_body<BWD, NV, 4, R>(a, b, w, tok, part);
  } else {
    const int s = ncoop + 4 * (b - ncoop) + w;
    if (s < a.n) pool_team_body<BWD, NV, 1, R>(a, s, 0, tok, part);
  }
}

}  // namespace

static int pool_check(const nnr_pool_args* p) {
  if (!p || !p->x || p->n <= 0) return NNR_ERR_ARG;
  if ((p->D & 3) || p->D > 4 * 64 * MAXV_ALL || (p->ldx & 3)) return NNR_ERR_UNSUPPORTED;
  if (p->L > 64 * MAXT) return NNR_ERR_UNSUPPORTED;
  // every per-sequence / per-token vector is read or written as float4: a leading dimension that is in use must keep rows 16-byte aligned
  auto odd = [](const void* ptr, int ld) { return ptr != nullptr && (ld & 3) != 0; };
  if (odd(p->v, p->ldv) || odd(p->out, p->ldo) || odd(p->add_in, p->ldadd) || odd(p->dout, p->lddo) || odd(p->dout2, p->lddo2) ||
      odd(p->dx, p->lddx) || odd(p->dv, p->lddv) || odd(p->dout_b, p->lddo_b) || odd(p->v_b, p->ldv_b)) return NNR_ERR_UNSUPPORTED;
  if (p->packed && (!p->off || !p->slen || !p->order)) return NNR_ERR_ARG;
  if (!p->v && !p->score && !p->alpha && !p->th) return NNR_ERR_ARG;
  if (p->th && (!p->w2 || p->A <= 0 || p->A > 256 || (p->A & 3) || (p->ldth & 3))) return NNR_ERR_UNSUPPORTED;
  return NNR_OK;
}

static PoolArgs to_args(const nnr_pool_args* p) {
  PoolArgs a;
  a.x = p->x; a.ldx = p->ldx; a.D = p->D; a.n = p->n; a.L = p->L; a.packed = p->packed;
  a.off = p->off; a.slen = p->slen; a.order = p->order; a.mask = p->mask; a.mask_div = p->mask_div > 0 ? p->mask_div : 1;
  a.score = p->score; a.v = p->v; a.ldv = p->ldv; a.scale = p->v ? p->scale : 1.f;
  a.alpha = p->alpha; a.out = p->out; a.ldo = p->ldo; a.add_in = p->add_in; a.ldadd = p->ldadd;
  a.dout = p->dout; a.lddo = p->lddo; a.dout2 = p->dout2; a.lddo2 = p->lddo2;
  a.dx = p->dx; a.lddx = p->lddx; a.dx_accumulate = p->dx_accumulate; a.dscore = p->dscore; a.dv = p->dv; a.lddv = p->lddv;
  a.th = p->th; a.ldth = p->ldth; a.A = p->A; a.w2 = p->w2;
  a.alpha_b = p->alpha_b; a.dout_b = p->dout_b; a.lddo_b = p->lddo_b; a.dscore_b = p->dscore_b; a.v_b = p->v_b; a.ldv_b = p->ldv_b; a.scale_b = p->scale_b;
  return a;
}

template <bool BWD>
static int pool_launch(const nnr_pool_args* p, hipStream_t stream) {
  const PoolArgs a = to_args(p);
  const dim3 grid(p->n), block(256);
  const int nv = (p->D + 3) / 4;
  // packed streams: the register-resident team kernels, 8 rows per wave (4 waves / SIMD, single-wave teams up to 8 tokens, shared up to 32);
  // anything else: one streaming workgroup per sequence
  if (p->packed && nv <= 128 && p->L <= 128) {
    if (nv <= 64) hipLaunchKernelGGL((pool_packed_kernel<BWD, 1, 8>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((pool_packed_kernel<BWD, 2, 8>), grid, block, 0, stream, a);
    NNR_CHECK_LAUNCH();
    return NNR_OK;
  }
  if (nv <= 64) hipLaunchKernelGGL((pool_kernel<BWD, 1, 4>), grid, block, 0, stream, a);
  else if (nv <= 128) hipLaunchKernelGGL((pool_kernel<BWD, 2, 4>), grid, block, 0, stream, a);
  else if (nv <= 256) hipLaunchKernelGGL((pool_kernel<BWD, 4, 2>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((pool_kernel<BWD, 5, 2>), grid, block, 0, stream, a);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_attn_pool_fwd(const nnr_pool_args* p, hipStream_t stream) {
  int rc = pool_check(p);
  if (rc != NNR_OK) return rc;
  if (!p->out || (!p->v && !p->score && !p->th)) return NNR_ERR_ARG;
  return pool_launch<false>(p, stream);
}

extern "C" int nnr_attn_pool_bwd(const nnr_pool_args* p, hipStream_t stream) {
  int rc = pool_check(p);
  if (rc != NNR_OK) return rc;
  if (!p->dout || !p->alpha) return NNR_ERR_ARG;
  if (p->alpha_b && (!p->dout_b || !p->dscore_b || !p->v_b || !p->dx || p->dx_accumulate)) return NNR_ERR_ARG;
  return pool_launch<true>(p, stream);
}
