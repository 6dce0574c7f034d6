// Per-title personalised attention: PNE's word-level attention (newsEncoders.py:359-360), i.e. layers.CandidateAttention
// (layers.py:225-232, tanh) with the query taken through an index map.  Per title i (L word positions) and position t:
//   a[i,t]     = w2 . tanh(Qf[i,t,:] + P[uidx[i],:])     Qf = feature projection [n*L, A], P = query projection + bias [U, A] (two GEMMs)
//   alpha[i,:] = softmax_t(mask[i,t] ? a[i,t] : -1e9)    (a title without any live position: 1/L over ALL L positions, as the reference)
//   out[i,:]   = sum_t alpha[i,t] * feat[i,t,:]
// cand_attn.hip expresses this as B' = n, N = 1, H = L, which is degenerate for its work split (one workgroup per (title, 256-column slice)
// with 32 busy threads on the scores, one workgroup per title in the backward pass, and the query projection carried for n rows where U
// exist).  Here:
//   one WAVE per title, four titles per 256-thread workgroup; every reduction of either direction is wave-local, no LDS, no barrier;
//   P[uidx[i]] and w2 stay in registers across the title's positions (up to PA_NA chunks of 64 lanes: A <= 256 * V);
//   only LIVE positions are read (Qf rows and feature rows; masks are arbitrary bit patterns, walked through a 64-bit ballot), four
//   positions in flight per trip; the scores are reduced inside the wave and held one per lane (L <= 64);
//   an all-masked title needs no score at all (alpha = 1/L exactly) and passes no gradient to the scores (the mask is tested, not alpha);
//   backward  one pass per title: d alpha, softmax backward, dfeat rows (zero rows where alpha is zero), then the Qf rows once more for
//             dQf (zero rows where masked) with the title's dP share and dw2 share accumulated in registers and written to the title's OWN
//             workspace row.  Follow-ups: dP[u] = sum of the rows of u's titles in ascending title order (one wave per (user, 64 columns)),
//             and nnr_colsum's fixed-order reduction for dw2.  No float atomics into shared destinations: same inputs, same bits.
// An out-of-range uidx entry means "no query": P = 0 for that title and its row joins no dP row; nothing outside P / dP is touched.
#include "common.h"

namespace {

constexpr int PA_NA = 4;                          // 64-lane chunks of the A axis held in registers
constexpr int PA_UR = 4;                          // positions in flight per trip


// the next (up to) PA_UR set bits of `bits`, lowest first; t[u] = -1 when there are fewer
__device__ __forceinline__ void pa_take(unsigned long long& bits, int (&t)[PA_UR]) {
#pragma unroll
  for (int u = 0; u < PA_UR; ++u) {
    t[u] = bits ? __ffsll((long long)bits) - 1 : -1;
    bits &= bits - 1;
  }
}

// live positions of title i as a bit set (wave-uniform); `none` = the mask has no live position
__device__ __forceinline__ unsigned long long pa_live(const uint8_t* __restrict__ mask, long i, int L, int lane, bool* none) {
  const unsigned long long all = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
  if (!mask) { *none = false; return all; }
  const unsigned long long b = __ballot(lane < L && mask[i * L + lane] != 0);
  *none = b == 0ull;
  return b;
}

template <int V>
__global__ __launch_bounds__(256) void pers_attn_fwd_kernel(const float* __restrict__ Qf, const float* __restrict__ P, const int* __restrict__ uidx,
                                                            int U, const float* __restrict__ w2, const float* __restrict__ feat, int ldf,
                                                            const uint8_t* __restrict__ mask, int n, int L, int A, int F,
                                                            float* __restrict__ alpha, float* __restrict__ out) {
  typedef typename vec_t<V>::type vec;
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                                      // (wave-uniform; the kernel has no barrier)
  bool none;
  const unsigned long long live = pa_live(mask, i, L, lane, &none);
  const int ncA = A / V, ncF = F / V;
  float a;                                                                 // alpha of position `lane`
  if (none) {
    a = lane < L ? 1.f / (float)L : 0.f;
  } else {
    const int u = uidx[i];
    const bool has_q = u >= 0 && u < U;
    vec p[PA_NA], w[PA_NA];
#pragma unroll
    for (int c = 0; c < PA_NA; ++c) {
      const int col = c * 64 + lane;
      const bool in = col < ncA;
      p[c] = (in && has_q) ? *reinterpret_cast<const vec*>(P + (long)u * A + (long)col * V) : vzero<V>();
      w[c] = in ? *reinterpret_cast<const vec*>(w2 + (long)col * V) : vzero<V>();
    }
    float s = -INFINITY;
    const float* qb = Qf + i * L * A;
    unsigned long long bits = live;
    while (bits) {
      int t[PA_UR];
      pa_take(bits, t);
      float part[PA_UR];
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) part[r] = 0.f;
#pragma unroll
      for (int c = 0; c < PA_NA; ++c) {
        if (c * 64 >= ncA) break;
        const int col = c * 64 + lane;
        vec q[PA_UR];
#pragma unroll
        for (int r = 0; r < PA_UR; ++r)
          q[r] = (col < ncA && t[r] >= 0) ? *reinterpret_cast<const vec*>(qb + (long)t[r] * A + (long)col * V) : vzero<V>();
#pragma unroll
        for (int r = 0; r < PA_UR; ++r) part[r] += vdot(w[c], vtanh(q[r] + p[c]));      // (w = 0 beyond A)
      }
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) {
        const float v = wave_sum(part[r]);
        if (lane == t[r]) s = v;
      }
    }
    const float m = wave_max(s);
    const float e = ((live >> lane) & 1ull) ? expf(s - m) : 0.f;
    a = e / wave_sum(e);
  }
  if (lane < L) alpha[i * L + lane] = a;
  // out[i, cols] = sum over the positions with a weight (all L of an all-masked title) of alpha[t] feat[i, t, cols]
  const unsigned long long used = none ? (L >= 64 ? ~0ull : ((1ull << L) - 1ull)) : live;
  const float* fb = feat + i * L * (long)ldf;
  for (int c0 = 0; c0 < ncF; c0 += 64) {
    const int col = c0 + lane;
    const bool in = col < ncF;
    vec acc = vzero<V>();
    unsigned long long bits = used;
    while (bits) {
      int t[PA_UR];
      pa_take(bits, t);
      vec f[PA_UR];
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) f[r] = (in && t[r] >= 0) ? *reinterpret_cast<const vec*>(fb + (long)t[r] * ldf + (long)col * V) : vzero<V>();
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) acc += __shfl(a, t[r] < 0 ? 0 : t[r], 64) * f[r];
    }
    if (in) *reinterpret_cast<vec*>(out + i * F + (long)col * V) = acc;
  }
}

// one pass per title: dfeat rows, dQf rows, the title's dP share (rows_p[i]) and dw2 share (rows_w[i])
template <int V>
__global__ __launch_bounds__(256) void pers_attn_bwd_kernel(const float* __restrict__ Qf, const float* __restrict__ P, const int* __restrict__ uidx,
                                                            int U, const float* __restrict__ w2, const float* __restrict__ feat, int ldf,
                                                            const uint8_t* __restrict__ mask, const float* __restrict__ alpha,
                                                            const float* __restrict__ dout, int n, int L, int A, int F,
                                                            float* __restrict__ dQf, float* __restrict__ dfeat, float* __restrict__ rows_p,
                                                            float* __restrict__ rows_w) {
  typedef typename vec_t<V>::type vec;
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  bool none;
  const unsigned long long live = pa_live(mask, i, L, lane, &none);
  const int ncA = A / V, ncF = F / V;
  const float a = lane < L ? alpha[i * L + lane] : 0.f;
  // d alpha[t] = <dout[i], feat[i, t]> for the live positions; dfeat[i, t] = alpha[t] dout[i] for every position
  float dal = 0.f;
  const float* fb = feat + i * L * (long)ldf;
  float* dfb = dfeat + i * L * (long)F;
  const float* dr = dout + i * F;
  for (int t0 = 0; t0 < L; t0 += PA_UR) {
    float part[PA_UR], at[PA_UR];
    bool lv[PA_UR];
#pragma unroll
    for (int r = 0; r < PA_UR; ++r) {
      part[r] = 0.f;
      at[r] = __shfl(a, (t0 + r) & 63, 64);
      lv[r] = t0 + r < L && !none && ((live >> (t0 + r)) & 1ull);
    }
    for (int c0 = 0; c0 < ncF; c0 += 64) {
      const int col = c0 + lane;
      const bool in = col < ncF;
      const vec d = in ? *reinterpret_cast<const vec*>(dr + (long)col * V) : vzero<V>();
      vec f[PA_UR];
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) f[r] = (in && lv[r]) ? *reinterpret_cast<const vec*>(fb + (long)(t0 + r) * ldf + (long)col * V) : vzero<V>();
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) {
        part[r] += vdot(d, f[r]);
        if (in && t0 + r < L) *reinterpret_cast<vec*>(dfb + (long)(t0 + r) * F + (long)col * V) = at[r] * d;
      }
    }
#pragma unroll
    for (int r = 0; r < PA_UR; ++r) {
      const float v = wave_sum(part[r]);
      if (lane == t0 + r) dal = v;
    }
  }
  // softmax backward; a masked position's score is a constant (masked_fill): no gradient, also in an all-masked title
  const bool mine = !none && ((live >> lane) & 1ull);
  const float dot = wave_sum(mine ? a * dal : 0.f);
  const float da = mine ? a * (dal - dot) : 0.f;
  // dQf[i, t, k] = da[t] w2[k] (1 - th^2), zero rows where masked; dP share = sum_t of it; dw2 share = sum_t da[t] th
  const int u = uidx[i];
  const bool has_q = u >= 0 && u < U;
  vec p[PA_NA], w[PA_NA], accP[PA_NA], accW[PA_NA];
#pragma unroll
  for (int c = 0; c < PA_NA; ++c) {
    const int col = c * 64 + lane;
    const bool in = col < ncA;
    p[c] = (in && has_q) ? *reinterpret_cast<const vec*>(P + (long)u * A + (long)col * V) : vzero<V>();
    w[c] = in ? *reinterpret_cast<const vec*>(w2 + (long)col * V) : vzero<V>();
    accP[c] = vzero<V>();
    accW[c] = vzero<V>();
  }
  const float* qb = Qf + i * L * A;
  float* dqb = dQf + i * L * A;
  for (int t0 = 0; t0 < L; t0 += PA_UR) {
    float dt[PA_UR];
    bool lv[PA_UR];
#pragma unroll
    for (int r = 0; r < PA_UR; ++r) {
      dt[r] = __shfl(da, (t0 + r) & 63, 64);
      lv[r] = t0 + r < L && !none && ((live >> (t0 + r)) & 1ull);
    }
#pragma unroll
    for (int c = 0; c < PA_NA; ++c) {
      if (c * 64 >= ncA) break;
      const int col = c * 64 + lane;
      const bool in = col < ncA;
      vec q[PA_UR];
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) q[r] = (in && lv[r]) ? *reinterpret_cast<const vec*>(qb + (long)(t0 + r) * A + (long)col * V) : vzero<V>();
#pragma unroll
      for (int r = 0; r < PA_UR; ++r) {
        vec g = vzero<V>();
        if (lv[r]) {
          const vec th = vtanh(q[r] + p[c]);
          g = dt[r] * w[c] * (1.f - th * th);
          accP[c] += g;
          accW[c] += dt[r] * th;
        }
        if (in && t0 + r < L) *reinterpret_cast<vec*>(dqb + (long)(t0 + r) * A + (long)col * V) = g;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < PA_NA; ++c) {
    const int col = c * 64 + lane;
    if (col < ncA) {
      *reinterpret_cast<vec*>(rows_p + i * A + (long)col * V) = accP[c];
      *reinterpret_cast<vec*>(rows_w + i * A + (long)col * V) = accW[c];
    }
  }
}

// dP[u, k] = sum over the titles i with uidx[i] == u, in ascending i, of rows_p[i, k]: one wave per (user, 64 columns); the index scan is
// wave-uniform.  A user without titles gets a zero row; an index outside [0, U) matches no user.
__global__ __launch_bounds__(256) void pers_attn_user_sum_kernel(const float* __restrict__ rows_p, const int* __restrict__ uidx, int n, int U, int A,
                                                                 int SA, float* __restrict__ dP) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int u = wv / SA, k = (wv - u * SA) * 64 + lane;
  if (u >= U) return;
  float acc = 0.f;
  for (int i0 = 0; i0 < n; i0 += 8) {
    int id[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) id[r] = i0 + r < n ? uidx[i0 + r] : -1;
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (id[r] == u && k < A) acc += rows_p[(long)(i0 + r) * A + k];
  }
  if (k < A) dP[(long)u * A + k] = acc;
}


}  // namespace

extern "C" int nnr_pers_attn_ws_floats(int n, int L, int A) {
  if (n < 1 || L < 1 || A < 1) return NNR_ERR_ARG;
  const long f = 2L * n * A + nnr_slot_workspace_floats(A);
  return f > 0x7fffffffL ? NNR_ERR_UNSUPPORTED : (int)f;
}

extern "C" int nnr_pers_attn_fwd(const float* Qf, const float* P, const int* uidx, int U, const float* w2, const float* feat, int ldf,
                                 const uint8_t* mask, int n, int L, int A, int F, float* alpha, float* out, hipStream_t stream) {
  if (!Qf || !P || !uidx || !w2 || !feat || !alpha || !out || U < 1 || n < 1 || L < 1 || A < 1 || F < 1 || ldf < F) return NNR_ERR_ARG;
  const int V = (!(A & 3) && !(F & 3) && !(ldf & 3) && al16(Qf) && al16(P) && al16(w2) && al16(feat) && al16(out)) ? 4 : 1;
  if (L > 64 || A > 64 * PA_NA * V) return NNR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  if (V == 4)
    hipLaunchKernelGGL((pers_attn_fwd_kernel<4>), grid, block, 0, stream, Qf, P, uidx, U, w2, feat, ldf, mask, n, L, A, F, alpha, out);
  else
    hipLaunchKernelGGL((pers_attn_fwd_kernel<1>), grid, block, 0, stream, Qf, P, uidx, U, w2, feat, ldf, mask, n, L, A, F, alpha, out);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_pers_attn_bwd(const float* Qf, const float* P, const int* uidx, int U, const float* w2, const float* feat, int ldf,
                                 const uint8_t* mask, const float* alpha, const float* dout, int n, int L, int A, int F, float* dP, float* dQf,
                                 float* dfeat, float* ws, float* dw2, hipStream_t stream) {
  if (!Qf || !P || !uidx || !w2 || !feat || !alpha || !dout || !dP || !dQf || !dfeat || !ws || !dw2 || U < 1 || n < 1 || L < 1 || A < 1 ||
      F < 1 || ldf < F)
    return NNR_ERR_ARG;
  if (nnr_pers_attn_ws_floats(n, L, A) < 0) return NNR_ERR_UNSUPPORTED;
  float* rows_p = ws;
  float* rows_w = ws + (long)n * A;
  float* slots = rows_w + (long)n * A;
  const int V = (!(A & 3) && !(F & 3) && !(ldf & 3) && al16(Qf) && al16(P) && al16(w2) && al16(feat) && al16(dout) &&
                 al16(dQf) && al16(dfeat) && al16(ws)) ? 4 : 1;
  const int SA = (A + 63) / 64;
  if (L > 64 || A > 64 * PA_NA * V || (long)U * SA > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  if (V == 4)
    hipLaunchKernelGGL((pers_attn_bwd_kernel<4>), grid, block, 0, stream, Qf, P, uidx, U, w2, feat, ldf, mask, alpha, dout, n, L, A, F, dQf,
                       dfeat, rows_p, rows_w);
  else
    hipLaunchKernelGGL((pers_attn_bwd_kernel<1>), grid, block, 0, stream, Qf, P, uidx, U, w2, feat, ldf, mask, alpha, dout, n, L, A, F, dQf,
                       dfeat, rows_p, rows_w);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(pers_attn_user_sum_kernel, dim3((unsigned)(((long)U * SA + 3) / 4)), block, 0, stream, (const float*)rows_p, uidx, n, U, A, SA,
                     dP);
  NNR_CHECK_LAUNCH();
  // dw2[k] += sum over the n title rows, in nnr_colsum's fixed order (own slot rows, then the slot reduction)
  return nnr_colsum(rows_w, A, nullptr, n, A, dw2, slots, stream);
}
