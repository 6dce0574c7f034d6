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
//     The reduction is csrc/sorted_rows.h's (chunks of WB_BCH, WB_FL gradient rows in flight, plain adds).  Both streams go through one
//     sorted list, so a table row has exactly one writer per launch: no float atomics, same bits every run.
//   * cosine_loss_kernel: logits[b, n] = <u_b, v_bn> / (|u_b| |v_bn|), loss = mean_b(-log_softmax(logits)[b, 0]) as a fixed-order sum
//     (the last workgroup to arrive adds the per-sample terms in index order, as click_loss_kernel does), d loss / d logits, d user (the sum
//     over the N candidates in ascending order) and d news.  One workgroup per sample.  A zero-norm row gives the reference's 0 / 0 = NaN.
//   * tanh_drop_bwd_kernel: dz = mask(dy) * (1 - t^2) behind y = dropout(tanh(z)), t = tanh(z) (functional.LinearFn with ACT_TANH).
#include "sorted_rows.h"

namespace {

constexpr int WB_MAXE = 1024;    // floats per table row
constexpr int WB_MAXL = 4096;    // positions per row of a stream
constexpr int WB_CH = 128;       // positions per forward work item: two ballots
constexpr int WB_FL = 4;         // table rows in flight per wave (forward) / gradient rows (backward)
constexpr int WB_BCH = 64;       // sorted occurrences per backward wave
constexpr int COS_MAXN = 64;

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

// ---- backward: csrc/sorted_rows.h over the sorted occurrences of both streams.  An entry is a position p of `tok`; it adds keep * scale * w *
// dout[stacked row], the dropout index being the forward's ((r * L + j) * E + col) within the occurrence's stream
struct WbagRows {
  struct Rec { int row, b; unsigned q; float w; };
  static constexpr int NV = 1;
  const float* dout;
  const int* poss;
  long cap, cap_a;
  const Stream &sa, &sb;                                           // (the kernel's arguments)
  int E;
  uint32_t thr, hhi_a, hhi_b;
  float scale;
  bool lo;                                                         // every dropout index below 2^32
  __device__ WbagRows(const float* dout_, const int* poss_, long cap_, const Stream& sa_, const Stream& sb_, int E_, uint32_t thr_, float scale_)
      : dout(dout_), poss(poss_), cap(cap_), cap_a((long)sa_.n * sa_.L), sa(sa_), sb(sb_), E(E_), thr(thr_), hhi_a(nnr_hash32(sa_.seed)),
        hhi_b(nnr_hash32(sb_.seed)), scale(scale_), lo((uint64_t)max(cap_a, cap_ - cap_a) * (uint64_t)E_ <= 0xFFFFFFFFull) {}
  __device__ Rec pad() const { return {0, 0, 0u, 0.f}; }
  __device__ Rec record(long i, bool live) const {
    if (!live) return pad();
    const long p = min(max((long)poss[i], 0L), cap - 1);
    const int b = p >= cap_a;
    const Stream& s = b ? sb : sa;
    const long q = b ? p - cap_a : p;
    const int r = (int)(q / s.L), j = (int)(q - (long)r * s.L);
    const int src = s.sel ? s.sel[r] : r;
    return {(b ? sa.n : 0) + r, b, (unsigned)q, (unsigned)src < (unsigned)s.R ? s.w[(long)src * s.L + j] : 0.f};
  }
  __device__ int nv() const { return 1; }
  __device__ const float* row(const Rec& e, int) const { return dout + (long)e.row * E; }
  struct Pre { uint32_t seed, hhi; uint64_t base; float w; };      // the occurrence's stream seed and first dropout index, its weight
  __device__ Pre prep(const Rec& e) const { return {e.b ? sb.seed : sa.seed, e.b ? hhi_b : hhi_a, (uint64_t)e.q * (uint64_t)E, e.w}; }
  __device__ float addend(const Pre& o, int col, bool in, const float (&v)[1]) const {
    float g = in ? v[0] * o.w : 0.f;
    if (thr) g = (in && (lo ? keep_lo(o.hhi, o.base + col, thr) : nnr_keep(o.seed, o.base + col, thr))) ? g * scale : 0.f;
    return g;
  }
};

template <int MAXJ>
__global__ __launch_bounds__(256) void wbag_bwd_kernel(const float* __restrict__ dout, const unsigned* __restrict__ keys, const int* __restrict__ poss,
                                                       long cap, Stream sa, Stream sb, unsigned V, int E, uint32_t thr, float scale,
                                                       float* __restrict__ dtable, float* __restrict__ partial) {
  sorted_rows::pass1<WB_BCH, MAXJ, WB_FL, false, true>(WbagRows(dout, poss, cap, sa, sb, E, thr, scale), keys, cap, V, E, dtable, partial);
}

template <int MAXJ>
__global__ __launch_bounds__(256) void wbag_bwd_fix_kernel(const unsigned* __restrict__ keys, long cap, unsigned V, int E, float* __restrict__ dtable,
                                                           const float* __restrict__ partial) {
  sorted_rows::fix<WB_BCH, MAXJ, (MAXJ >= 16 ? 4 : 8), false>(keys, cap, V, E, dtable, partial);   // partial rows in flight: at most 64 registers
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
  const unsigned blocks = sorted_rows::blocks(cap, WB_BCH);
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
  return sorted_rows::ws_floats(cap, WB_BCH, bwd_maxj(E));
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
