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
//     (r = pos / (La + Lb)): n rows that stay in L2, not one row per token.  One wave sums a chunk of 32 sorted occurrences in list
//     order; a word whose occurrences lie inside one chunk is added to its table row by that wave alone with a plain read-add-write, a
//     run that crosses a chunk boundary is stored as a partial row, and the workgroup whose chunk holds the START of such a word adds
//     the partial rows in chunk order and writes the table row.  Every table row has exactly one writer: no float atomics, same bits
//     every run.  (The chunk / partial geometry and the boundary rules are csrc/sort.hip's: keep the two copies in step.)
//   * row_dist_fwd_kernel / row_dist_bwd_kernel: aux[r] = coef * ||a[r] - b[r]||_2 and its backward into both operands; one wave per row.
// Row loads are 16-byte vectors when E % 4 == 0, 8-byte vectors when E % 2 == 0 (a row of E = 50 floats starts on an 8-byte boundary
// only), scalars otherwise.
#include "common.h"

namespace {

constexpr int BAG_MAXL = 128;      // positions per stream: two ballots
constexpr int BAG_MAXE = 320;      // floats per row: 5 columns per lane in the backward pass
constexpr int BAG_CH = 32;         // sorted occurrences per wave
constexpr int BAG_MAXJ = 5;
constexpr int BAG_FL = 8;          // rows in flight per wave
constexpr int BAG_PITCH = 64 * BAG_MAXJ;

template <int VEC> struct VecT;
template <> struct VecT<4> { typedef float4 type; };
template <> struct VecT<2> { typedef float2 type; };
template <> struct VecT<1> { typedef float type; };

template <int VEC> __device__ __forceinline__ void vec_get(const typename VecT<VEC>::type& v, float (&f)[VEC]);
template <> __device__ __forceinline__ void vec_get<4>(const float4& v, float (&f)[4]) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
template <> __device__ __forceinline__ void vec_get<2>(const float2& v, float (&f)[2]) { f[0] = v.x; f[1] = v.y; }
template <> __device__ __forceinline__ void vec_get<1>(const float& v, float (&f)[1]) { f[0] = v; }

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

// ---- backward, pass 1: one wave per chunk of BAG_CH sorted occurrences
__global__ __launch_bounds__(256) void bag_mean_bwd_kernel(const float* __restrict__ dout, int lddo, const float* __restrict__ outp, int ldo,
                                                           int off_a, int off_b, const float* __restrict__ count,
                                                           const unsigned* __restrict__ keys, const int* __restrict__ poss, long cap, int La,
                                                           int Lb, int n, unsigned V, int E, int separate, float* __restrict__ dtable,
                                                           float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long c = blockIdx.x * 4L + wv;
  const long p0 = c * BAG_CH;
  if (p0 >= cap) return;
  const long p1 = min(cap, p0 + BAG_CH);
  const int cnt = (int)(p1 - p0);
  const int Lt = La + Lb;
  unsigned myk = V;
  int myr = 0, myo = off_a;
  float myc = 1.f;
  if (lane < cnt) {
    myk = keys[p0 + lane];
    if (myk < V) {
      const int p = poss[p0 + lane];
      const int r = min(max(p / Lt, 0), n - 1);
      const bool isb = (p - r * Lt) >= La;
      myr = r;
      myo = (separate && isb) ? off_b : off_a;
      myc = count[(separate && isb) ? n + r : r];
    }
  }
  const unsigned k0 = __shfl(myk, 0, 64);
  if (k0 >= V) return;                                            // sorted: nothing but pad entries from here on
  const unsigned prevK = p0 > 0 ? keys[p0 - 1] : 0xFFFFFFFFu;     // (0xFFFFFFFF equals no valid key)
  const unsigned nextK = p1 < cap ? keys[p1] : 0xFFFFFFFFu;
  float acc[BAG_MAXJ];
#pragma unroll
  for (int j = 0; j < BAG_MAXJ; ++j) acc[j] = 0.f;
  unsigned run_key = k0;
  bool first = true;
  auto flush = [&](bool open_right) {
    const bool open_left = first && prevK == run_key;
    if (!open_left && !open_right) {                              // the whole segment of this word: this wave is the row's only writer
#pragma unroll
      for (int j = 0; j < BAG_MAXJ; ++j) {
        const int col = lane + 64 * j;
        if (col < E) dtable[(long)run_key * E + col] += acc[j];
      }
    } else {
      float* dst = partial + (c * 2 + (first ? 0 : 1)) * (long)BAG_PITCH;
#pragma unroll
      for (int j = 0; j < BAG_MAXJ; ++j) dst[lane + 64 * j] = acc[j];
    }
  };
  bool done = false;
  const int elast = E - 1;
  for (int i0 = 0; i0 < cnt && !done; i0 += BAG_FL) {
    float v[BAG_FL][BAG_MAXJ], o[BAG_FL][BAG_MAXJ];
    unsigned kk[BAG_FL];
    int rr[BAG_FL], oo[BAG_FL];
    float cc[BAG_FL];
#pragma unroll
    for (int u = 0; u < BAG_FL; ++u) {
      const int i = i0 + u;                                       // (< 64: lanes >= cnt hold the pad key, row 0 and count 1)
      kk[u] = __shfl(myk, i, 64);
      rr[u] = __shfl(myr, i, 64);
      oo[u] = __shfl(myo, i, 64);
      cc[u] = __shfl(myc, i, 64);
    }
#pragma unroll
    for (int u = 0; u < BAG_FL; ++u) {
      const float* src = dout + (long)rr[u] * lddo + oo[u];
#pragma unroll
      for (int j = 0; j < BAG_MAXJ; ++j) v[u][j] = src[min(lane + 64 * j, elast)];
      if (outp) {
        const float* so = outp + (long)rr[u] * ldo + oo[u];
#pragma unroll
        for (int j = 0; j < BAG_MAXJ; ++j) o[u][j] = so[min(lane + 64 * j, elast)];
      }
    }
#pragma unroll
    for (int u = 0; u < BAG_FL; ++u) {
      if (done) break;
      if (kk[u] >= V) { done = true; break; }
      if (kk[u] != run_key) {
        flush(false);
        run_key = kk[u];
        first = false;
#pragma unroll
        for (int j = 0; j < BAG_MAXJ; ++j) acc[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < BAG_MAXJ; ++j) {
        const int col = lane + 64 * j;
        float g = col < E ? v[u][j] : 0.f;
        if (outp) g = col < E ? g * o[u][j] * (1.f - o[u][j]) : 0.f;
        acc[j] += g / cc[u];
      }
    }
  }
  flush(nextK == run_key);                                        // (a chunk that ran into pad entries has nextK = pad: closed)
}

// ---- backward, pass 2: the workgroup of the chunk in which a multi-chunk word STARTS adds its partial rows in chunk order
__global__ __launch_bounds__(256) void bag_mean_bwd_fix_kernel(const unsigned* __restrict__ keys, long cap, unsigned V, int E,
                                                               float* __restrict__ dtable, const float* __restrict__ partial) {
  __shared__ float red[4][BAG_PITCH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long nchunks = (cap + BAG_CH - 1) / BAG_CH;
  for (int ci = 0; ci < 4; ++ci) {
    const long c = blockIdx.x * 4L + ci;
    const long p0 = c * BAG_CH;
    if (p0 >= cap) break;                                          // (uniform over the workgroup, like every branch below)
    const long p1 = min(cap, p0 + BAG_CH);
    const unsigned k0 = keys[p0];
    if (k0 >= V) break;
    const unsigned prevK = p0 > 0 ? keys[p0 - 1] : 0xFFFFFFFFu;
    const unsigned kl = keys[p1 - 1];
    const unsigned nextK = p1 < cap ? keys[p1] : 0xFFFFFFFFu;
    for (int cand = 0; cand < 2; ++cand) {
      // cand 0: the chunk's first run, if the word STARTS here and runs on into the next chunk; cand 1: its last run, likewise
      const unsigned key = cand == 0 ? k0 : kl;
      const bool own = cand == 0 ? (prevK != k0 && kl == k0 && nextK == k0) : (kl != k0 && kl < V && nextK == kl);
      if (!own) continue;
      float acc[BAG_MAXJ];
#pragma unroll
      for (int j = 0; j < BAG_MAXJ; ++j) acc[j] = 0.f;
      long cc = c + 1;
      while (true) {
        const bool cont = (cc + lane < nchunks) && keys[(cc + lane) * BAG_CH] == key;
        const unsigned long long m = __ballot(cont);
        const int nc = (m == ~0ull) ? 64 : __builtin_ctzll(~m);   // chunks cc .. cc + nc - 1 begin with this word: their slot 0 is its partial
        for (int q = wv; q < nc; q += 32) {                        // this wave: chunks q, q + 4, ..., q + 28 of the window, in order
          float v[8][BAG_MAXJ];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float* sp = partial + ((cc + min(q + 4 * u, nc - 1)) * 2) * (long)BAG_PITCH;
#pragma unroll
            for (int j = 0; j < BAG_MAXJ; ++j) v[u][j] = sp[lane + 64 * j];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (q + 4 * u < nc) {
#pragma unroll
              for (int j = 0; j < BAG_MAXJ; ++j) acc[j] += v[u][j];
            }
          }
        }
        cc += nc;
        if (nc < 64) break;
      }
#pragma unroll
      for (int j = 0; j < BAG_MAXJ; ++j) red[wv][lane + 64 * j] = acc[j];
      __syncthreads();
      if (wv == 0) {
        const float* src = partial + (c * 2 + cand) * (long)BAG_PITCH;      // the run's own part in its first chunk
#pragma unroll
        for (int j = 0; j < BAG_MAXJ; ++j) {
          const int col = lane + 64 * j;
          const float t = (((src[col] + red[0][col]) + red[1][col]) + red[2][col]) + red[3][col];
          if (col < E) dtable[(long)key * E + col] += t;
        }
      }
      __syncthreads();
    }
  }
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
  return cap <= 0 ? 0 : (size_t)((cap + BAG_CH - 1) / BAG_CH) * 2 * BAG_PITCH;
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
  const long nchunks = (cap + BAG_CH - 1) / BAG_CH;
  const unsigned blocks = (unsigned)((nchunks + 3) / 4);
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
