// DSSM baseline (general_recommendation_methods/DSSM_model.py:29-36, DSSM_main.py:63): the two weighted bags of word-embedding rows, their
// table gradient, and the cosine click head with its loss.  The reference gathers [B, 3200, 512] and [B, N, 200, 512] rows, multiplies
// them by the tf-idf weights, runs dropout over them and sums: 419 MB + 131 MB of buffers at batch 64 for a [64 + 320, 512] result.  Here no
// [tokens, E] buffer exists in either direction:
//   * wbag_fwd_kernel: both streams (a = users, b = news) in one launch into one stacked output [na + nb, E].  A row is cut into chunks of
//     WB_CH positions; one wave sums one (row, chunk): it reads the chunk's ids and weights, compacts the live positions into LDS (ballot +
//     prefix count, ascending) and adds weight * table row in that order, four rows in flight, fp32 with a compensation term.  A row of
//     one chunk is written to `out` directly; otherwise the wave stores a partial row and wbag_combine_kernel adds a row's partials in
//     ascending chunk order.  64 user rows of 3200 positions are 1600 waves, not 64.  The dropout of DSSM_model.py:29-30 is applied
//     inside the sum: keep(seed, ((r * L + j) * E + e)) per element, two hashes per float4; p = 0 skips the hash.
//     A position with w == 0 contributes nothing and its table row is NOT read (the reference computes 0 * row, which differs only for a
//     row that holds a non-finite value); an id outside [0, V) contributes a zero row and receives no gradient; a selector entry outside
//     the term-vector table selects an empty row.  The launch also writes the occurrence keys (word id of a live position, -1 otherwise)
//     that nnr_token_sort turns into the (word, position) list of the backward pass.
//   * wbag_bwd_kernel / wbag_bwd_fix_kernel: dtable[word] += sum over the word's live occurrences, in list order, of keep * scale * w *
//     dout[row of the occurrence]: the gradient row is read through the sorted position from the na + nb rows of dout (they stay in L2).
//     One wave sums a chunk of WB_BCH sorted occurrences; a word inside one chunk is added to its table row by that wave alone (plain
//     read-add-write), a run that crosses a chunk boundary goes through partial rows and the fix-up pass, which adds them in chunk order:
//     the geometry and the boundary rules are csrc/bag.hip's and csrc/sort.hip's.  Both streams go through one sorted list, so a table row
//     has exactly one writer per launch: no float atomics, same bits every run.
//   * cosine_loss_kernel: logits[b, n] = <u_b, v_bn> / (|u_b| |v_bn|), loss = mean_b(-log_softmax(logits)[b, 0]) as a fixed-order sum
//     (the last workgroup to arrive adds the per-sample terms in index order, as click_loss_kernel does), d loss / d logits, d user (the sum
//     over the N candidates in ascending order) and d news.  One workgroup per sample.  A zero-norm row gives the reference's 0 / 0 = NaN.
//   * tanh_drop_bwd_kernel: dz = mask(dy) * (1 - t^2) behind y = dropout(tanh(z)), t = tanh(z) (functional.LinearFn with ACT_TANH).
#include "common.h"

namespace {

constexpr int WB_MAXE = 1024;    // floats per table row
constexpr int WB_MAXL = 4096;    // positions per row of a stream
constexpr int WB_CH = 128;       // positions per forward work item: two ballots
constexpr int WB_FL = 4;         // table rows in flight per wave (forward) / gradient rows (backward)
constexpr int WB_BCH = 64;       // sorted occurrences per backward wave
constexpr int COS_MAXN = 64;

template <int VEC> struct VecT;
template <> struct VecT<4> { typedef float4 type; };
template <> struct VecT<2> { typedef float2 type; };
template <> struct VecT<1> { typedef float type; };
template <int VEC> __device__ __forceinline__ void vec_get(const typename VecT<VEC>::type& v, float (&f)[VEC]);
template <> __device__ __forceinline__ void vec_get<4>(const float4& v, float (&f)[4]) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
template <> __device__ __forceinline__ void vec_get<2>(const float2& v, float (&f)[2]) { f[0] = v.x; f[1] = v.y; }
template <> __device__ __forceinline__ void vec_get<1>(const float& v, float (&f)[1]) { f[0] = v; }
template <int VEC> __device__ __forceinline__ typename VecT<VEC>::type vec_zero();
template <> __device__ __forceinline__ float4 vec_zero<4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ float2 vec_zero<2>() { return make_float2(0.f, 0.f); }
template <> __device__ __forceinline__ float vec_zero<1>() { return 0.f; }

// nnr_keep / nnr_keep4 (common.h) for an index below 2^32, given hhi = nnr_hash32(seed): the hash of the index's high word is then the same
// for every element of the launch and leaves the per-element work (one hash per pair of elements instead of two)
__device__ __forceinline__ bool keep_lo(uint32_t hhi, uint64_t idx, uint32_t thresh) {
  const uint32_t h = nnr_hash32((uint32_t)(idx >> 1) ^ hhi);
  return ((h >> (16u * (uint32_t)(idx & 1))) & 0xFFFFu) >= thresh;
}
__device__ __forceinline__ void keep4_lo(uint32_t hhi, uint64_t idx4, uint32_t thresh, bool (&k)[4]) {
  const uint32_t pr = (uint32_t)(idx4 >> 1);
  const uint32_t h0 = nnr_hash32(pr ^ hhi), h1 = nnr_hash32((pr + 1u) ^ hhi);
  k[0] = (h0 & 0xFFFFu) >= thresh; k[1] = (h0 >> 16) >= thresh; k[2] = (h1 & 0xFFFFu) >= thresh; k[3] = (h1 >> 16) >= thresh;
}

// one stream of a weighted-bag call (kernel argument, not part of the C-ABI)
struct Stream {
  const int* ids;        // [R, L] (forward only)
  const float* w;        // [R, L]
  const int* sel;        // [n] rows of the table, or NULL: identity
  int n, L, R, nchunk;
  uint32_t seed;
};

static inline int nchunks_of(int L) { return (L + WB_CH - 1) / WB_CH; }

// ---- forward: one wave per (row, chunk of WB_CH positions)
template <int VEC, int NJ>
__global__ __launch_bounds__(256) void wbag_fwd_kernel(const float* __restrict__ table, int V, int E, Stream sa, Stream sb, uint32_t thr, float scale,
                                                       float* __restrict__ out, int* __restrict__ tok, float* __restrict__ ws) {
  typedef typename VecT<VEC>::type vec_t;
  __shared__ int l_id[4][WB_CH];
  __shared__ int l_pos[4][WB_CH];
  __shared__ float l_w[4][WB_CH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long units_a = (long)sa.n * sa.nchunk;
  const long units = units_a + (long)sb.n * sb.nchunk;
  const long u = blockIdx.x * 4L + wv;
  const bool valid = u < units;
  const bool isb = valid && u >= units_a;
  const int* ids = isb ? sb.ids : sa.ids;
  const float* wts = isb ? sb.w : sa.w;
  const int* sel = isb ? sb.sel : sa.sel;
  const int L = isb ? sb.L : sa.L, R = isb ? sb.R : sa.R, nchunk = isb ? sb.nchunk : sa.nchunk;
  const uint32_t seed = isb ? sb.seed : sa.seed;
  const uint32_t hhi = nnr_hash32(seed);
  const bool lo = (uint64_t)(isb ? sb.n : sa.n) * (uint64_t)L * (uint64_t)E <= 0xFFFFFFFFull;      // every dropout index of the stream below 2^32
  int r = 0, c = 0, cnt = 0;
  if (valid) {
    const long uu = isb ? u - units_a : u;
    r = (int)(uu / nchunk);
    c = (int)(uu - (long)r * nchunk);
    const int src = sel ? sel[r] : r;
    const bool row_ok = (unsigned)src < (unsigned)R;              // a selector entry outside the table: an empty row
    const long tok_base = (isb ? (long)sa.n * sa.L : 0L) + (long)r * L;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int h = 0; h < WB_CH / 64; ++h) {
      const int pos = c * WB_CH + lane + 64 * h;
      int id = -1;
      float w = 0.f;
      bool live = false;
      if (pos < L) {
        if (row_ok) {
          id = ids[(long)src * L + pos];
          w = wts[(long)src * L + pos];
        }
        live = row_ok && w != 0.f && (unsigned)id < (unsigned)V;   // (a NaN weight is live, as in the reference's product)
        if (tok) tok[tok_base + pos] = live ? id : -1;
      }
      const unsigned long long b = __ballot(live);
      if (live) {
        const int k = cnt + __popcll(b & below);
        l_id[wv][k] = id;
        l_pos[wv][k] = pos;
        l_w[wv][k] = w;
      }
      cnt += __popcll(b);
    }
  }
  __syncthreads();
  if (!valid) return;

  // compensated (Kahan) sum in list order, as bag_mean_fwd_kernel: the products are rounded once each, the running sum adds no more
  float acc[NJ][VEC], comp[NJ][VEC];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[j][e] = comp[j][e] = 0.f;
  for (int k = 0; k < cnt; k += WB_FL) {
    // every load is issued before any is used; entries past the end of the list repeat the last one and are skipped below
    int id[WB_FL], ps[WB_FL];
    float w[WB_FL];
    vec_t v[WB_FL][NJ];
#pragma unroll
    for (int q = 0; q < WB_FL; ++q) {
      const int kk = min(k + q, cnt - 1);
      id[q] = l_id[wv][kk];
      ps[q] = l_pos[wv][kk];
      w[q] = l_w[wv][kk];
    }
#pragma unroll
    for (int q = 0; q < WB_FL; ++q) {
      const float* src = table + (long)id[q] * E;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = (lane + 64 * j) * VEC;
        v[q][j] = col < E ? *reinterpret_cast<const vec_t*>(src + col) : vec_zero<VEC>();
      }
    }
#pragma unroll
    for (int q = 0; q < WB_FL; ++q) {
      if (k + q >= cnt) break;                                     // (wave-uniform)
      const uint64_t base = ((uint64_t)r * (uint64_t)L + (uint64_t)ps[q]) * (uint64_t)E;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = (lane + 64 * j) * VEC;
        float f[VEC];
        vec_get<VEC>(v[q][j], f);
        bool kp[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) kp[e] = true;
        if (thr) {
          if constexpr (VEC == 4) {                                // E % 4 == 0 on this path: the index is a multiple of 4
            if (lo) keep4_lo(hhi, base + col, thr, kp);
            else nnr_keep4(seed, base + col, thr, kp);
          } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) kp[e] = lo ? keep_lo(hhi, base + col + e, thr) : nnr_keep(seed, base + col + e, thr);
          }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float x = f[e] * w[q];
          if (thr) x = kp[e] ? x * scale : 0.f;
          const float y = x - comp[j][e];
          const float t = acc[j][e] + y;
          comp[j][e] = (t - acc[j][e]) - y;
          acc[j][e] = t;
        }
      }
    }
  }
  float* dst = nchunk == 1 ? out + ((long)(isb ? sa.n : 0) + r) * E : ws + u * E;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = (lane + 64 * j) * VEC;
    if (col < E) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) dst[col + e] = acc[j][e];
    }
  }
}

// ---- forward, pass 2: out[r] = the row's partial rows in ascending chunk order (rows of one chunk were written by pass 1)
__global__ __launch_bounds__(256) void wbag_combine_kernel(const float* __restrict__ ws, int E, int na, int nchunk_a, int nb, int nchunk_b,
                                                           float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)(na + nb) * E) return;
  const int r = (int)(i / E), e = (int)(i - (long)r * E);
  long base;
  int nc;
  if (r < na) {
    nc = nchunk_a;
    base = (long)r * nchunk_a;
  } else {
    nc = nchunk_b;
    base = (long)na * nchunk_a + (long)(r - na) * nchunk_b;
  }
  if (nc == 1) return;
  out[i] = partial_rows_sum(ws + base * E, nc, E, e);
}

// ---- backward, pass 1: one wave per chunk of WB_BCH sorted occurrences; lane + 64 j is the column
template <int MAXJ>
__global__ __launch_bounds__(256) void wbag_bwd_kernel(const float* __restrict__ dout, const unsigned* __restrict__ keys, const int* __restrict__ poss,
                                                       long cap, Stream sa, Stream sb, unsigned V, int E, uint32_t thr, float scale,
                                                       float* __restrict__ dtable, float* __restrict__ partial) {
  constexpr int PITCH = 64 * MAXJ;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long c = blockIdx.x * 4L + wv;
  const long p0 = c * WB_BCH;
  if (p0 >= cap) return;
  const long p1 = min(cap, p0 + WB_BCH);
  const int cnt = (int)(p1 - p0);
  const long cap_a = (long)sa.n * sa.L;
  const uint32_t hhi_a = nnr_hash32(sa.seed), hhi_b = nnr_hash32(sb.seed);
  const bool lo = (uint64_t)max(cap_a, cap - cap_a) * (uint64_t)E <= 0xFFFFFFFFull;                 // every dropout index below 2^32
  unsigned myk = V, myq = 0;
  int myrow = 0, myb = 0;
  float myw = 0.f;
  if (lane < cnt) {
    myk = keys[p0 + lane];
    if (myk < V) {
      const long p = min(max((long)poss[p0 + lane], 0L), cap - 1);
      myb = p >= cap_a;
      const Stream& s = myb ? sb : sa;
      const long q = myb ? p - cap_a : p;
      const int r = (int)(q / s.L), j = (int)(q - (long)r * s.L);
      const int src = s.sel ? s.sel[r] : r;
      myw = (unsigned)src < (unsigned)s.R ? s.w[(long)src * s.L + j] : 0.f;
      myrow = (myb ? sa.n : 0) + r;
      myq = (unsigned)q;
    }
  }
  const unsigned k0 = __shfl(myk, 0, 64);
  if (k0 >= V) return;                                            // sorted: nothing but pad entries from here on
  const unsigned prevK = p0 > 0 ? keys[p0 - 1] : 0xFFFFFFFFu;     // (0xFFFFFFFF equals no valid key)
  const unsigned nextK = p1 < cap ? keys[p1] : 0xFFFFFFFFu;
  float acc[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
  unsigned run_key = k0;
  bool first = true;
  auto flush = [&](bool open_right) {
    const bool open_left = first && prevK == run_key;
    if (!open_left && !open_right) {                              // the whole segment of this word: this wave is the row's only writer
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int col = lane + 64 * j;
        if (col < E) dtable[(long)run_key * E + col] += acc[j];
      }
    } else {
      float* dst = partial + (c * 2 + (first ? 0 : 1)) * (long)PITCH;
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) dst[lane + 64 * j] = acc[j];
    }
  };
  bool done = false;
  const int elast = E - 1;
  for (int i0 = 0; i0 < cnt && !done; i0 += WB_FL) {
    float v[WB_FL][MAXJ];
    unsigned kk[WB_FL], qq[WB_FL];
    int rr[WB_FL], bb[WB_FL];
    float ww[WB_FL];
#pragma unroll
    for (int u = 0; u < WB_FL; ++u) {
      const int i = i0 + u;                                       // (< 64 + WB_FL: __shfl wraps; lanes >= cnt hold the pad key and row 0)
      kk[u] = i < cnt ? __shfl(myk, i, 64) : V;
      rr[u] = __shfl(myrow, i, 64);
      bb[u] = __shfl(myb, i, 64);
      qq[u] = __shfl(myq, i, 64);
      ww[u] = __shfl(myw, i, 64);
    }
#pragma unroll
    for (int u = 0; u < WB_FL; ++u) {
      const float* src = dout + (long)rr[u] * E;
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) v[u][j] = src[min(lane + 64 * j, elast)];
    }
#pragma unroll
    for (int u = 0; u < WB_FL; ++u) {
      if (done) break;
      if (kk[u] >= V) { done = true; break; }
      if (kk[u] != run_key) {
        flush(false);
        run_key = kk[u];
        first = false;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
      }
      const uint32_t seed = bb[u] ? sb.seed : sa.seed, hhi = bb[u] ? hhi_b : hhi_a;
      const uint64_t base = (uint64_t)qq[u] * (uint64_t)E;
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int col = lane + 64 * j;
        float g = col < E ? v[u][j] * ww[u] : 0.f;
        if (thr) g = (col < E && (lo ? keep_lo(hhi, base + col, thr) : nnr_keep(seed, base + col, thr))) ? g * scale : 0.f;
        acc[j] += g;
      }
    }
  }
  flush(nextK == run_key);                                        // (a chunk that ran into pad entries has nextK = pad: closed)
}

// ---- backward, pass 2: the workgroup of the chunk in which a multi-chunk word STARTS adds its partial rows in chunk order
template <int MAXJ>
__global__ __launch_bounds__(256) void wbag_bwd_fix_kernel(const unsigned* __restrict__ keys, long cap, unsigned V, int E, float* __restrict__ dtable,
                                                           const float* __restrict__ partial) {
  constexpr int PITCH = 64 * MAXJ;
  constexpr int U = MAXJ >= 16 ? 4 : 8;                           // partial rows in flight per wave
  __shared__ float red[4][PITCH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long nchunks = (cap + WB_BCH - 1) / WB_BCH;
  for (int ci = 0; ci < 4; ++ci) {
    const long c = blockIdx.x * 4L + ci;
    const long p0 = c * WB_BCH;
    if (p0 >= cap) break;                                          // (uniform over the workgroup, like every branch below)
    const long p1 = min(cap, p0 + WB_BCH);
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
      float acc[MAXJ];
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
      long cc = c + 1;
      while (true) {
        const bool cont = (cc + lane < nchunks) && keys[(cc + lane) * WB_BCH] == key;
        const unsigned long long m = __ballot(cont);
        const int nc = (m == ~0ull) ? 64 : __builtin_ctzll(~m);   // chunks cc .. cc + nc - 1 begin with this word: their slot 0 is its partial
        for (int q = wv; q < nc; q += 4 * U) {                     // this wave: chunks q, q + 4, ... of the window, in order
          float v[U][MAXJ];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float* sp = partial + ((cc + min(q + 4 * u, nc - 1)) * 2) * (long)PITCH;
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) v[u][j] = sp[lane + 64 * j];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (q + 4 * u < nc) {
#pragma unroll
              for (int j = 0; j < MAXJ; ++j) acc[j] += v[u][j];
            }
          }
        }
        cc += nc;
        if (nc < 64) break;
      }
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) red[wv][lane + 64 * j] = acc[j];
      __syncthreads();
      if (wv == 0) {
        const float* src = partial + (c * 2 + cand) * (long)PITCH;          // the run's own part in its first chunk
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
          const int col = lane + 64 * j;
          const float t = (((src[col] + red[0][col]) + red[1][col]) + red[2][col]) + red[3][col];
          if (col < E) dtable[(long)key * E + col] += t;
        }
      }
      __syncthreads();
    }
  }
}

// ---- cosine click head + loss, one workgroup per sample
__device__ unsigned g_cosine_arrived;
__global__ __launch_bounds__(256) void cosine_loss_kernel(const float* __restrict__ user, const float* __restrict__ news, int B, int N, int F,
                                                          float* __restrict__ logits, float* __restrict__ loss, float* __restrict__ dlogits,
                                                          float* __restrict__ duser, float* __restrict__ dnews, float* __restrict__ terms) {
  __shared__ float l[COS_MAXN], d[COS_MAXN], vv[COS_MAXN], dotp[COS_MAXN];
  __shared__ float uu_s;
  __shared__ float part[256];
  __shared__ bool last;
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* u = user + (long)b * F;
  const float* v = news + (long)b * N * F;
  if (w == 0) {
    float s = 0.f;
    for (int x = lane; x < F; x += 64) s += u[x] * u[x];
    s = wave_sum(s);
    if (lane == 0) uu_s = s;
  }
  for (int n = w; n < N; n += 4) {
    float p = 0.f, s = 0.f;
    for (int x = lane; x < F; x += 64) {
      const float a = v[(long)n * F + x];
      p += u[x] * a;
      s += a * a;
    }
    p = wave_sum(p);
    s = wave_sum(s);
    if (lane == 0) { dotp[n] = p; vv[n] = s; }
  }
  __syncthreads();
  const float uu = uu_s;
  const float nu = sqrtf(uu);
  if (threadIdx.x < N) {
    const int n = threadIdx.x;
    const float lg = dotp[n] / (nu * sqrtf(vv[n]));               // DSSM_model.py:35-36; 0 / 0 for a zero row, as there
    l[n] = lg;
    logits[(long)b * N + n] = lg;
  }
  __syncthreads();
  if (!loss && !dlogits && !duser) return;                        // the eval call: logits only
  if (threadIdx.x == 0) {
    float m = -INFINITY;
    for (int n = 0; n < N; ++n) m = fmaxf(m, l[n]);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += expf(l[n] - m);
    const float lse = m + logf(s);
    for (int n = 0; n < N; ++n) {
      const float dv = (expf(l[n] - lse) - (n == 0 ? 1.f : 0.f)) / (float)B;
      d[n] = dv;
      if (dlogits) dlogits[(long)b * N + n] = dv;
    }
    if (loss) terms[b] = lse - l[0];
  }
  __syncthreads();
  if (duser) {
    // d l_n / d u = v_n / (|u| |v_n|) - l_n u / |u|^2 ;  d l_n / d v_n = u / (|u| |v_n|) - l_n v_n / |v_n|^2
    for (int x = threadIdx.x; x < F; x += 256) {
      const float ux = u[x];
      float du = 0.f;
      for (int n = 0; n < N; ++n) {                               // ascending n: a fixed-order sum
        const float a = v[(long)n * F + x];
        const float inv = 1.f / (nu * sqrtf(vv[n]));
        du += d[n] * (a * inv - l[n] * ux / uu);
        dnews[((long)b * N + n) * F + x] = d[n] * (ux * inv - l[n] * a / vv[n]);
      }
      duser[(long)b * F + x] = du;
    }
  }
  if (!loss) return;
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(&g_cosine_arrived, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  float t = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) t += __builtin_nontemporal_load(&terms[i]);
  part[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *loss = part[0] / (float)B;
    g_cosine_arrived = 0;                                  // (launches of one process are stream-ordered)
  }
}

// ---- backward of  y = dropout(tanh(z))  given t = tanh(z):  dz = mask(dy) * (1 - t^2)
__global__ void tanh_drop_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ t, float* __restrict__ dz, long n, uint32_t seed,
                                     uint32_t thr, float scale) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float m = nnr_keep(seed, (uint64_t)i, thr) ? scale : 0.f;
    const float v = t[i];
    dz[i] = dy[i] * m * (1.f - v * v);
  }
}

template <int VEC, int NJ>
int launch_fwd(const float* table, int V, int E, const Stream& sa, const Stream& sb, float p, float* out, int* tok, float* ws, hipStream_t stream) {
  const long units = (long)sa.n * sa.nchunk + (long)sb.n * sb.nchunk;
  const float sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
  hipLaunchKernelGGL((wbag_fwd_kernel<VEC, NJ>), dim3((unsigned)((units + 3) / 4)), dim3(256), 0, stream, table, V, E, sa, sb, nnr_drop_thresh(p), sc,
                     out, tok, ws);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

template <int MAXJ>
int launch_bwd(const float* dout, const unsigned* keys, const int* poss, long cap, const Stream& sa, const Stream& sb, int V, int E, float p,
               float* dtable, float* partial, hipStream_t stream) {
  const long nchunks = (cap + WB_BCH - 1) / WB_BCH;
  const unsigned blocks = (unsigned)((nchunks + 3) / 4);
  const float sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
  hipLaunchKernelGGL(wbag_bwd_kernel<MAXJ>, dim3(blocks), dim3(256), 0, stream, dout, keys, poss, cap, sa, sb, (unsigned)V, E, nnr_drop_thresh(p), sc,
                     dtable, partial);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(wbag_bwd_fix_kernel<MAXJ>, dim3(blocks), dim3(256), 0, stream, keys, cap, (unsigned)V, E, dtable, partial);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

static inline int bwd_maxj(int E) { return E <= 256 ? 4 : (E <= 512 ? 8 : 16); }

}  // namespace

extern "C" int nnr_wbag_dims(int E, int La, int Lb, int* chunk, int* nchunk_a, int* nchunk_b) {
  if (chunk) *chunk = WB_CH;
  if (E < 1 || E > WB_MAXE || La < 1 || La > WB_MAXL || Lb < 0 || Lb > WB_MAXL) return NNR_ERR_UNSUPPORTED;
  if (nchunk_a) *nchunk_a = nchunks_of(La);
  if (nchunk_b) *nchunk_b = nchunks_of(Lb);
  return NNR_OK;
}

extern "C" size_t nnr_wbag_fwd_ws_floats(int na, int La, int nb, int Lb, int E) {
  if (na < 0 || nb < 0 || La < 1 || Lb < 0 || E < 1) return 0;
  return ((size_t)na * nchunks_of(La) + (size_t)nb * nchunks_of(Lb)) * (size_t)E;
}

extern "C" int nnr_wbag_fwd(const float* table, int V, int E, const int* ids_a, const float* w_a, const int* sel_a, int Ra, int na, int La,
                            const int* ids_b, const float* w_b, const int* sel_b, int Rb, int nb, int Lb, float p, uint32_t seed_a,
                            uint32_t seed_b, float* out, int* tok, float* ws, hipStream_t stream) {
  if (!table || !out || !ws || V <= 0 || na < 0 || nb < 0 || Ra < 0 || Rb < 0 || (na > 0 && (!ids_a || !w_a)) || (nb > 0 && (!ids_b || !w_b)) ||
      (!sel_a && Ra < na) || (!sel_b && Rb < nb) || (nb > 0 && Lb < 1) || p < 0.f || p >= 1.f)
    return NNR_ERR_ARG;
  if (nnr_wbag_dims(E, La, Lb, nullptr, nullptr, nullptr) != NNR_OK) return NNR_ERR_UNSUPPORTED;
  if ((long)na * La + (long)nb * Lb > 0x7FFFFFFFL) return NNR_ERR_UNSUPPORTED;      // positions are int32 (the sort's values)
  if (na + nb == 0) return NNR_OK;
  const Stream sa = {ids_a, w_a, sel_a, na, La, Ra, nchunks_of(La), seed_a};
  const Stream sb = {ids_b, w_b, sel_b, nb, nb > 0 ? Lb : 1, Rb, nb > 0 ? nchunks_of(Lb) : 1, seed_b};
  int rc;
  // the vector width the rows' alignment allows (a row starts at table + id * E floats)
  const uintptr_t base = (uintptr_t)table;
  if (E % 4 == 0 && base % 16 == 0) {
    if (E <= 256) rc = launch_fwd<4, 1>(table, V, E, sa, sb, p, out, tok, ws, stream);
    else if (E <= 512) rc = launch_fwd<4, 2>(table, V, E, sa, sb, p, out, tok, ws, stream);
    else rc = launch_fwd<4, 4>(table, V, E, sa, sb, p, out, tok, ws, stream);
  } else if (E % 2 == 0 && base % 8 == 0) {
    rc = launch_fwd<2, 8>(table, V, E, sa, sb, p, out, tok, ws, stream);
  } else {
    rc = launch_fwd<1, 16>(table, V, E, sa, sb, p, out, tok, ws, stream);
  }
  if (rc != NNR_OK) return rc;
  if (sa.nchunk > 1 || sb.nchunk > 1) {
    const long total = (long)(na + nb) * E;
    hipLaunchKernelGGL(wbag_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ws, E, na, sa.nchunk, nb, sb.nchunk, out);
    NNR_CHECK_LAUNCH();
  }
  return NNR_OK;
}

extern "C" size_t nnr_wbag_bwd_ws_floats(long cap, int E) {
  if (cap <= 0 || E < 1 || E > WB_MAXE) return 0;
  return (size_t)((cap + WB_BCH - 1) / WB_BCH) * 2 * 64 * bwd_maxj(E);
}

extern "C" int nnr_wbag_bwd(const float* dout, const unsigned* keys_sorted, const int* pos_sorted, long cap, const float* w_a, const int* sel_a,
                            int Ra, int na, int La, const float* w_b, const int* sel_b, int Rb, int nb, int Lb, int V, int E, float p,
                            uint32_t seed_a, uint32_t seed_b, float* dtable_accum, float* partial_ws, hipStream_t stream) {
  if (!dout || !keys_sorted || !pos_sorted || !dtable_accum || !partial_ws || V <= 0 || na < 0 || nb < 0 || Ra < 0 || Rb < 0 || (na > 0 && !w_a) ||
      (nb > 0 && !w_b) || (!sel_a && Ra < na) || (!sel_b && Rb < nb) || (nb > 0 && Lb < 1) || p < 0.f || p >= 1.f)
    return NNR_ERR_ARG;
  if (nnr_wbag_dims(E, La, Lb, nullptr, nullptr, nullptr) != NNR_OK) return NNR_ERR_UNSUPPORTED;
  if (cap != (long)na * La + (long)nb * Lb) return NNR_ERR_ARG;
  if (cap > 0x7FFFFFFFL) return NNR_ERR_UNSUPPORTED;
  if (cap == 0) return NNR_OK;
  const Stream sa = {nullptr, w_a, sel_a, na, La, Ra, 0, seed_a};
  const Stream sb = {nullptr, w_b, sel_b, nb, nb > 0 ? Lb : 1, Rb, 0, seed_b};
  switch (bwd_maxj(E)) {
    case 4: return launch_bwd<4>(dout, keys_sorted, pos_sorted, cap, sa, sb, V, E, p, dtable_accum, partial_ws, stream);
    case 8: return launch_bwd<8>(dout, keys_sorted, pos_sorted, cap, sa, sb, V, E, p, dtable_accum, partial_ws, stream);
    default: return launch_bwd<16>(dout, keys_sorted, pos_sorted, cap, sa, sb, V, E, p, dtable_accum, partial_ws, stream);
  }
}

extern "C" int nnr_cosine_loss(const float* user, const float* news, int B, int N, int F, float* logits, float* loss, float* dlogits, float* duser,
                               float* dnews, float* ws, hipStream_t stream) {
  if (!user || !news || !logits || B <= 0 || N <= 0 || F <= 0 || ((duser == nullptr) != (dnews == nullptr)) || (loss && !ws)) return NNR_ERR_ARG;
  if (N > COS_MAXN) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cosine_loss_kernel, dim3(B), dim3(256), 0, stream, user, news, B, N, F, logits, loss, dlogits, duser, dnews, ws);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_tanh_drop_bwd(const float* dy, const float* t, float* dz, long n, float p, uint32_t seed, hipStream_t stream) {
  if (!dy || !t || !dz || n < 0 || p < 0.f || p >= 1.f) return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  const float sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
  hipLaunchKernelGGL(tanh_drop_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, stream, dy, t, dz, n, seed, nnr_drop_thresh(p), sc);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
