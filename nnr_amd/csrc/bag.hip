// Bag-of-words front of the DAE (newsEncoders.py:366-394) and Inception (newsEncoders.py:397-433) news encoders: a masked mean of
// word-embedding rows over the live positions of up to two token streams per news (title, abstract), its table gradient, and the
// DAE's reconstruction distance.  The reference gathers [n, L, E] rows, multiplies them by the mask and reduces; two thirds of those
// positions are padding.  Here no [tokens, E] buffer exists in either direction:
//   * bag_mean_fwd_kernel: one wave per news.  It reads the mask bytes and ids of both streams, compacts the ids of the live positions
//     into LDS (ballot + prefix count; stream a ascending, then stream b ascending), and adds the table rows of that list in list order,
//     four rows in flight, fp32 with a compensation term.  Joint mode (DAE): one sum over both streams / (count_a + count_b), sigmoid.  Separate mode (Inception):
//     one mean per stream into two column slices of one output buffer, after forcing position 0 live in place (newsEncoders.py:422-423).
//     The launch also writes the occurrence keys (word id of a live position, -1 otherwise) that nnr_token_sort turns into the list
//     of (word, position) pairs ordered by word for the backward pass, and the counts as floats.
//   * bag_mean_bwd_kernel / bag_mean_bwd_fix_kernel: dtable[w] += sum over the live occurrences (r, pos) of w of g[r] / count[r], with
//     g[r] = dout[r] (or dout[r] * out[r] * (1 - out[r]) behind the sigmoid) read from the owning news' row through the sorted position
//     (r = pos / (La + Lb)): n rows that stay in L2, not one row per token.  The reduction is csrc/sorted_rows.h's (chunks of 32, 8 rows
//     in flight in both passes, plain adds: every table row has exactly one writer, no float atomics, same bits every run).
//   * row_dist_fwd_kernel / row_dist_bwd_kernel: aux[r] = coef * ||a[r] - b[r]||_2 and its backward into both operands; one wave per row.
// Row loads are 16-byte vectors when E % 4 == 0, 8-byte vectors when E % 2 == 0 (a row of E = 50 floats starts on an 8-byte boundary
// only), scalars otherwise.
#include "sorted_rows.h"

namespace {

constexpr int BAG_MAXL = 128;      // positions per stream: two ballots
constexpr int BAG_MAXE = 320;      // floats per row: 5 columns per lane in the backward pass
constexpr int BAG_CH = 32;         // sorted occurrences per wave
constexpr int BAG_MAXJ = 5;
constexpr int BAG_FL = 8;          // rows in flight per wave, both passes

// ---- forward: one wave per news row
template <int VEC>
__global__ __launch_bounds__(256) void bag_mean_fwd_kernel(const float* __restrict__ table, int V, int E, const int* __restrict__ ids_a,
                                                           uint8_t* __restrict__ mask_a, int La, const int* __restrict__ ids_b,
                                                           uint8_t* __restrict__ mask_b, int Lb, int n, int separate, int act,
                                                           float* __restrict__ out, int ldo, int off_a, int off_b, float* __restrict__ count,
                                                           int* __restrict__ tok) {
  constexpr int NJ = (BAG_MAXE + 64 * VEC - 1) / (64 * VEC);
  typedef typename VecT<VEC>::type vec_t;
  __shared__ int list[4][2 * BAG_MAXL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long r = blockIdx.x * 4L + wv;
  const bool valid = r < n;
  const int Lt = La + Lb;
  int ca = 0, cb = 0;
  if (valid) {
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int* ids = s ? ids_b : ids_a;
      uint8_t* mask = s ? mask_b : mask_a;
      const int Lx = s ? Lb : La;
      int c = 0;
#pragma unroll
      for (int h = 0; h < BAG_MAXL / 64; ++h) {
        const int pos = lane + 64 * h;
        int id = -1;
        bool live = false;
        if (pos < Lx) {
          id = ids[r * Lx + pos];
          live = mask[r * Lx + pos] != 0;
          if (separate && pos == 0) {                            // newsEncoders.py:422-423, in place on the caller's tensor
            live = true;
            mask[r * Lx] = 1;
          }
          if ((unsigned)id >= (unsigned)V) id = -1;              // an id outside the table reads as a zero row and joins no gradient
          if (tok) tok[r * Lt + (s ? La : 0) + pos] = live ? id : -1;
        }
        const unsigned long long b = __ballot(live);
        if (live) list[wv][(s ? ca : 0) + c + __popcll(b & below)] = id;
        c += __popcll(b);
      }
      if (s) cb = c; else ca = c;
    }
  }
  __syncthreads();
  if (!valid) return;

  auto run = [&](int s0, int s1, float cnt, int off) {
    // compensated (Kahan) sum in list order: a news whose positions repeat one word adds the same row up to 256 times, and a plain
    // running sum is then k / 2 ulp off; two more adds per element cost nothing next to the row loads
    float acc[NJ][VEC], comp[NJ][VEC];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[j][e] = comp[j][e] = 0.f;
    for (int k = s0; k < s1; k += 4) {
      // four rows in flight: every load is issued before any is used; entries past the end of the list (and ids outside the table)
      // read row 0 / column 0 and are replaced by zeros
      int id[4];
      vec_t v[4][NJ];
#pragma unroll
      for (int u = 0; u < 4; ++u) id[u] = (k + u < s1) ? list[wv][k + u] : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* src = table + (long)(id[u] < 0 ? 0 : id[u]) * E;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int col = (lane + 64 * j) * VEC;
          v[u][j] = *reinterpret_cast<const vec_t*>(src + (col < E ? col : 0));
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool use = id[u] >= 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          float f[VEC];
          vec_get<VEC>(v[u][j], f);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float y = (use ? f[e] : 0.f) - comp[j][e];
            const float t = acc[j][e] + y;
            comp[j][e] = (t - acc[j][e]) - y;
            acc[j][e] = t;
          }
        }
      }
    }
    float* dst = out + r * ldo + off;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = (lane + 64 * j) * VEC;
      if (col < E) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float m = acc[j][e] / cnt;                       // plain IEEE: no live position gives the reference's 0 / 0
          dst[col + e] = act == 3 ? sigmoidf_(m) : m;
        }
      }
    }
  };
  if (separate) {
    run(0, ca, (float)ca, off_a);
    if (ids_b) run(ca, ca + cb, (float)cb, off_b);
    if (lane == 0) {
      count[r] = (float)ca;
      if (ids_b) count[n + r] = (float)cb;
    }
  } else {
    run(0, ca + cb, (float)(ca + cb), off_a);
    if (lane == 0) count[r] = (float)(ca + cb);
  }
}

// ---- backward: csrc/sorted_rows.h over the sorted occurrences.  An entry is a position p of `tok`; it adds g[r] / count with r = p / (La + Lb)
struct BagRows {
  struct Rec { int r, off; float cnt; };
  static constexpr int NV = 2;                                     // the gradient row, and the output row behind the sigmoid
  const float *dout, *outp, *count;
  const int* poss;
  int lddo, ldo, off_a, off_b, La, Lb, n, separate;
  __device__ Rec pad() const { return {0, off_a, 1.f}; }
  __device__ Rec record(long i, bool live) const {
    if (!live) return pad();
    const int Lt = La + Lb;
    const int p = poss[i];
    const int r = min(max(p / Lt, 0), n - 1);
    const bool isb = (p - r * Lt) >= La;
    return {r, (separate && isb) ? off_b : off_a, count[(separate && isb) ? n + r : r]};
  }
  __device__ int nv() const { return outp ? 2 : 1; }
  __device__ const Rec& prep(const Rec& e) const { return e; }
  __device__ const float* row(const Rec& e, int k) const { return k ? outp + (long)e.r * ldo + e.off : dout + (long)e.r * lddo + e.off; }
  __device__ float addend(const Rec& e, int, bool in, const float (&v)[2]) const {
    float g = in ? v[0] : 0.f;
    if (outp) g = in ? g * v[1] * (1.f - v[1]) : 0.f;
    return g / e.cnt;
  }
};

__global__ __launch_bounds__(256) void bag_mean_bwd_kernel(const float* __restrict__ dout, int lddo, const float* __restrict__ outp, int ldo,
                                                           int off_a, int off_b, const float* __restrict__ count,
                                                           const unsigned* __restrict__ keys, const int* __restrict__ poss, long cap, int La,
                                                           int Lb, int n, unsigned V, int E, int separate, float* __restrict__ dtable,
                                                           float* __restrict__ partial) {
  sorted_rows::pass1<BAG_CH, BAG_MAXJ, BAG_FL, false, false>(BagRows{dout, outp, count, poss, lddo, ldo, off_a, off_b, La, Lb, n, separate}, keys, cap, V, E,
                                                      dtable, partial);
}

__global__ __launch_bounds__(256) void bag_mean_bwd_fix_kernel(const unsigned* __restrict__ keys, long cap, unsigned V, int E,
                                                               float* __restrict__ dtable, const float* __restrict__ partial) {
  sorted_rows::fix<BAG_CH, BAG_MAXJ, BAG_FL, false>(keys, cap, V, E, dtable, partial);
}

// ---- aux[r] = coef * ||a[r] - b[r]||_2 ; one wave per row, fixed-order butterfly sum
__global__ __launch_bounds__(256) void row_dist_fwd_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, int n, int D,
                                                           float coef, float* __restrict__ dist, float* __restrict__ aux) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= n) return;
  float s = 0.f;
  for (int col = lane; col < D; col += 64) {
    const float d = a[r * lda + col] - b[r * ldb + col];
    s += d * d;
  }
  s = sqrtf(wave_sum(s));
  if (lane == 0) {
    dist[r] = s;
    aux[r] = coef * s;
  }
}

// ---- da[r] += u, db[r] -= u with u = gup[r] * coef * (a[r] - b[r]) / dist[r]; nothing at dist[r] == 0 (torch's 2-norm subgradient)
__global__ __launch_bounds__(256) void row_dist_bwd_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb,
                                                           const float* __restrict__ dist, const float* __restrict__ gup, int n, int D, float coef,
                                                           float* __restrict__ da, int ldda, float* __restrict__ db, int lddb) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= n) return;
  const float dd = dist[r];
  if (dd == 0.f) return;
  const float g = gup[r] * coef;
  for (int col = lane; col < D; col += 64) {
    const float u = g * (a[r * lda + col] - b[r * ldb + col]) / dd;
    da[r * ldda + col] += u;
    db[r * lddb + col] -= u;
  }
}

template <int VEC>
int launch_fwd(const float* table, int V, int E, const int* ids_a, uint8_t* mask_a, int La, const int* ids_b, uint8_t* mask_b, int Lb, int n,
               int separate, int act, float* out, int ldo, int off_a, int off_b, float* count, int* tok, hipStream_t stream) {
  hipLaunchKernelGGL(bag_mean_fwd_kernel<VEC>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, table, V, E, ids_a, mask_a, La, ids_b, mask_b, Lb,
                     n, separate, act, out, ldo, off_a, off_b, count, tok);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

}  // namespace

extern "C" int nnr_bag_mean_fwd(const float* table, int V, int E, const int* ids_a, uint8_t* mask_a, int La, const int* ids_b, uint8_t* mask_b,
                                int Lb, int n, int separate, int act, float* out, int ldo, int off_a, int off_b, float* count, int* tok,
                                hipStream_t stream) {
  if (!table || !ids_a || !mask_a || !out || !count || V <= 0 || E <= 0 || La <= 0 || n < 0 || (ids_b ? (!mask_b || Lb <= 0) : Lb != 0) ||
      off_a < 0 || off_b < 0 || off_a + E > ldo || (separate && ids_b && off_b + E > ldo) || (act != 0 && act != 3))
    return NNR_ERR_ARG;
  if (La > BAG_MAXL || Lb > BAG_MAXL || E > BAG_MAXE) return NNR_ERR_UNSUPPORTED;
  if (n == 0) return NNR_OK;
  // the vector width the rows' alignment allows (a row starts at table + id * E floats)
  const uintptr_t base = (uintptr_t)table;
  if (E % 4 == 0 && base % 16 == 0)
    return launch_fwd<4>(table, V, E, ids_a, mask_a, La, ids_b, mask_b, Lb, n, separate, act, out, ldo, off_a, off_b, count, tok, stream);
  if (E % 2 == 0 && base % 8 == 0)
    return launch_fwd<2>(table, V, E, ids_a, mask_a, La, ids_b, mask_b, Lb, n, separate, act, out, ldo, off_a, off_b, count, tok, stream);
  return launch_fwd<1>(table, V, E, ids_a, mask_a, La, ids_b, mask_b, Lb, n, separate, act, out, ldo, off_a, off_b, count, tok, stream);
}

extern "C" size_t nnr_bag_mean_bwd_ws_floats(long cap) {
  return sorted_rows::ws_floats(cap, BAG_CH, BAG_MAXJ);
}

extern "C" int nnr_bag_mean_bwd(const float* dout, int lddo, const float* out, int ldo, int off_a, int off_b, const float* count,
                                const unsigned* keys_sorted, const int* pos_sorted, long cap, int La, int Lb, int n, int V, int E, int separate,
                                int act, float* dtable_accum, float* partial_ws, hipStream_t stream) {
  if (!dout || !count || !keys_sorted || !pos_sorted || !dtable_accum || !partial_ws || cap < 0 || La <= 0 || Lb < 0 || n < 0 || V <= 0 || E <= 0 ||
      cap != (long)n * (La + Lb) || off_a < 0 || off_b < 0 || off_a + E > lddo || (separate && Lb > 0 && off_b + E > lddo) ||
      (act != 0 && act != 3) || (act == 3 && (!out || off_a + E > ldo || (separate && Lb > 0 && off_b + E > ldo))))
    return NNR_ERR_ARG;
  if (La > BAG_MAXL || Lb > BAG_MAXL || E > BAG_MAXE) return NNR_ERR_UNSUPPORTED;
  if (cap == 0) return NNR_OK;
  const unsigned blocks = sorted_rows::blocks(cap, BAG_CH);
  hipLaunchKernelGGL(bag_mean_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dout, lddo, act == 3 ? out : (const float*)nullptr, ldo, off_a, off_b,
                     count, keys_sorted, pos_sorted, cap, La, Lb, n, (unsigned)V, E, separate, dtable_accum, partial_ws);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bag_mean_bwd_fix_kernel, dim3(blocks), dim3(256), 0, stream, keys_sorted, cap, (unsigned)V, E, dtable_accum, partial_ws);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_row_dist_fwd(const float* a, int lda, const float* b, int ldb, int n, int D, float coef, float* dist, float* aux,
                                hipStream_t stream) {
  if (!a || !b || !dist || !aux || n < 0 || D <= 0 || lda < D || ldb < D) return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  hipLaunchKernelGGL(row_dist_fwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a, lda, b, ldb, n, D, coef, dist, aux);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_row_dist_bwd(const float* a, int lda, const float* b, int ldb, const float* dist, const float* gup, int n, int D, float coef,
                                float* da_accum, int ldda, float* db_accum, int lddb, hipStream_t stream) {
  if (!a || !b || !dist || !gup || !da_accum || !db_accum || n < 0 || D <= 0 || lda < D || ldb < D || ldda < D || lddb < D) return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  hipLaunchKernelGGL(row_dist_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a, lda, b, ldb, dist, gup, n, D, coef, da_accum, ldda,
                     db_accum, lddb);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
