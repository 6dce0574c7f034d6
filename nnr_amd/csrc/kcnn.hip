// KCNN (DKN) news encoder: the bandwidth kernels around its one convolution product (newsEncoders.py:203-241, layers.py:47-79 `naive`).
//
// The convolution Conv2d(E -> C, kernel [w, 3], padding [p, 0]) over the [E, L, 3] image of a title is ONE product on the GEMM family
// (csrc/gemm.hip, untouched) once its A operand is laid out as a padded image Xp[n][L + w - 1][3 E] (row = position, [channel j][e] inside
// a row, p = (w - 1) / 2 leading and w - 1 - p trailing zero rows per title): the window of output position t is the contiguous 3 w E
// floats that start at padded row t, i.e. a row-major A with lda = 3 E < K = 3 w E.  The kernels here build that image (word rows gathered
// straight from the table, tanh of the two projected knowledge channels, halo rows), take it apart again for the backward pass, do the
// relu + max over the first L - w + 1 positions with its dense gradient.  (The Conv2d weight's operand layouts: nnr_permute, csrc/misc.hip.)
// They move bytes: no MFMA, no LDS.
#include "common.h"

namespace {

constexpr int KCNN_MAX_ROWS = 255;   // L + w - 1: a position fits the uint8 arg (255 = "no positive maximum")
constexpr int KCNN_MAX_W = 8;
constexpr int KCNN_MAX_E = 1024;
constexpr int WM_TITLES = 8;         // titles per thread of window_max_bwd_kernel (one partial bias-gradient row per group)

static inline bool kcnn_dims_ok(int L, int E, int w) { return L + w - 1 <= KCNN_MAX_ROWS && w <= KCNN_MAX_W && E <= KCNN_MAX_E && L >= w; }

// one wave per padded row (i, s); VEC = 4: float4 accesses (E % 4 == 0, 16-byte aligned bases), VEC = 1: scalar
template <int VEC>
__global__ __launch_bounds__(256) void kcnn_image_fwd_kernel(const float* __restrict__ table, int V, const int* __restrict__ text,
                                                             const float* __restrict__ pre1, const float* __restrict__ pre2, long rows, int L, int E,
                                                             int w, float* __restrict__ Xp) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int Lp = L + w - 1, p = (w - 1) / 2;
  const long i = r / Lp;
  const int t = (int)(r - i * Lp) - p;
  float* __restrict__ dst = Xp + r * 3L * E;
  if (t < 0 || t >= L) {                                       // halo row
    if (VEC == 4) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      for (int q = lane; q < 3 * E / 4; q += 64) reinterpret_cast<f32x4*>(dst)[q] = z;
    } else {
      for (int q = lane; q < 3 * E; q += 64) dst[q] = 0.f;
    }
    return;
  }
  const long tok_row = i * L + t;
  const int id = text[tok_row];
  const bool live = id >= 0 && id < V;
  const float* __restrict__ src0 = table + (long)(live ? id : 0) * E;
  const float* __restrict__ s1 = pre1 + tok_row * E;
  const float* __restrict__ s2 = pre2 + tok_row * E;
  if (VEC == 4) {
    for (int q = lane; q < E / 4; q += 64) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (live) a = reinterpret_cast<const f32x4*>(src0)[q];
      const f32x4 b = reinterpret_cast<const f32x4*>(s1)[q], c = reinterpret_cast<const f32x4*>(s2)[q];
      f32x4 tb, tc;
#pragma unroll
      for (int u = 0; u < 4; ++u) { tb[u] = tanhf(b[u]); tc[u] = tanhf(c[u]); }
      reinterpret_cast<f32x4*>(dst)[q] = a;
      reinterpret_cast<f32x4*>(dst + E)[q] = tb;
      reinterpret_cast<f32x4*>(dst + 2 * E)[q] = tc;
    }
  } else {
    for (int q = lane; q < E; q += 64) {
      dst[q] = live ? src0[q] : 0.f;
      dst[E + q] = tanhf(s1[q]);
      dst[2 * E + q] = tanhf(s2[q]);
    }
  }
}

// one wave per title position (i, t): dx0 = dXp channel 0, dpre_j = dXp channel j * (1 - x_j^2); halo rows are not read
template <int VEC>
__global__ __launch_bounds__(256) void kcnn_image_bwd_kernel(const float* __restrict__ dXp, const float* __restrict__ Xp, long rows, int L, int E,
                                                             int w, float* __restrict__ dx0, float* __restrict__ dpre1, float* __restrict__ dpre2) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);        // r = i * L + t
  if (r >= rows) return;
  const int Lp = L + w - 1, p = (w - 1) / 2;
  const long i = r / L;
  const long pr = i * Lp + (r - i * L) + p;
  const float* __restrict__ g = dXp + pr * 3L * E;
  const float* __restrict__ x = Xp + pr * 3L * E;
  float* __restrict__ o0 = dx0 + r * E;
  float* __restrict__ o1 = dpre1 + r * E;
  float* __restrict__ o2 = dpre2 + r * E;
  if (VEC == 4) {
    for (int q = lane; q < E / 4; q += 64) {
      const f32x4 g0 = reinterpret_cast<const f32x4*>(g)[q], g1 = reinterpret_cast<const f32x4*>(g + E)[q], g2 = reinterpret_cast<const f32x4*>(g + 2 * E)[q];
      const f32x4 x1 = reinterpret_cast<const f32x4*>(x + E)[q], x2 = reinterpret_cast<const f32x4*>(x + 2 * E)[q];
      reinterpret_cast<f32x4*>(o0)[q] = g0;
      reinterpret_cast<f32x4*>(o1)[q] = g1 * (1.f - x1 * x1);
      reinterpret_cast<f32x4*>(o2)[q] = g2 * (1.f - x2 * x2);
    }
  } else {
    for (int q = lane; q < E; q += 64) {
      const float x1 = x[E + q], x2 = x[2 * E + q];
      o0[q] = g[q];
      o1[q] = g[E + q] * (1.f - x1 * x1);
      o2[q] = g[2 * E + q] * (1.f - x2 * x2);
    }
  }
}

// one thread per (title, channel), channels fastest: fl(z + b) over the first T positions, strict > keeps the lowest t on ties
__global__ __launch_bounds__(256) void window_max_fwd_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ bias, long total, int C,
                                                             int Lp, int T, float* __restrict__ out, uint8_t* __restrict__ arg) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= total) return;
  const long i = idx / C;
  const int c = (int)(idx - i * C);
  const float b = bias[c];
  const float* __restrict__ zp = z + i * Lp * (long)ldz + c;
  float m = 0.f;                                               // relu first: only a positive value can win
  int a = 255;
  for (int t = 0; t < T; ++t) {
    const float v = zp[(long)t * ldz] + b;
    if (v > m) { m = v; a = t; }
  }
  out[idx] = m;
  arg[idx] = (uint8_t)a;
}

// one thread per (group of WM_TITLES titles, channel): every element of dz written once; the group's bias-gradient partial to ws
__global__ __launch_bounds__(256) void window_max_bwd_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg, int n, int C, int Lp,
                                                             int lead, float* __restrict__ dz, float* __restrict__ ws) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  const int groups = (n + WM_TITLES - 1) / WM_TITLES;
  if (idx >= (long)groups * C) return;
  const int grp = (int)(idx / C), c = (int)(idx - (long)grp * C);
  if (grp == 0)
    for (int r = 0; r < lead; ++r) dz[(long)r * C + c] = 0.f;
  float part = 0.f;
  const int i1 = min(n, (grp + 1) * WM_TITLES);
  for (int i = grp * WM_TITLES; i < i1; ++i) {
    const int a = arg[(long)i * C + c];
    const float gv = g[(long)i * C + c];
    float* __restrict__ d = dz + ((long)lead + (long)i * Lp) * C + c;
    for (int s = 0; s < Lp; ++s) d[(long)s * C] = (s == a) ? gv : 0.f;
    if (a != 255) part += gv;
  }
  ws[(long)grp * C + c] = part;
}

}  // namespace

extern "C" int nnr_kcnn_image_fwd(const float* word_table, int V, const int* text, const float* pre1, const float* pre2, int n, int L, int E, int w,
                                  float* Xp, hipStream_t stream) {
  if (!word_table || !text || !pre1 || !pre2 || !Xp || V <= 0 || n < 0 || L <= 0 || E <= 0 || w <= 0) return NNR_ERR_ARG;
  if (!kcnn_dims_ok(L, E, w)) return NNR_ERR_UNSUPPORTED;
  if (n == 0) return NNR_OK;
  const long rows = (long)n * (L + w - 1);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (E % 4 == 0 && al16(word_table) && al16(pre1) && al16(pre2) && al16(Xp))
    hipLaunchKernelGGL(kcnn_image_fwd_kernel<4>, grid, dim3(256), 0, stream, word_table, V, text, pre1, pre2, rows, L, E, w, Xp);
  else
    hipLaunchKernelGGL(kcnn_image_fwd_kernel<1>, grid, dim3(256), 0, stream, word_table, V, text, pre1, pre2, rows, L, E, w, Xp);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_kcnn_image_bwd(const float* dXp, const float* Xp, int n, int L, int E, int w, float* dx0, float* dpre1, float* dpre2,
                                  hipStream_t stream) {
  if (!dXp || !Xp || !dx0 || !dpre1 || !dpre2 || n < 0 || L <= 0 || E <= 0 || w <= 0) return NNR_ERR_ARG;
  if (!kcnn_dims_ok(L, E, w)) return NNR_ERR_UNSUPPORTED;
  if (n == 0) return NNR_OK;
  const long rows = (long)n * L;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (E % 4 == 0 && al16(dXp) && al16(Xp) && al16(dx0) && al16(dpre1) && al16(dpre2))
    hipLaunchKernelGGL(kcnn_image_bwd_kernel<4>, grid, dim3(256), 0, stream, dXp, Xp, rows, L, E, w, dx0, dpre1, dpre2);
  else
    hipLaunchKernelGGL(kcnn_image_bwd_kernel<1>, grid, dim3(256), 0, stream, dXp, Xp, rows, L, E, w, dx0, dpre1, dpre2);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_window_max_fwd(const float* z, int ldz, const float* bias, int n, int C, int L, int w, float* out, uint8_t* arg,
                                  hipStream_t stream) {
  if (!z || !bias || !out || !arg || n < 0 || C <= 0 || L <= 0 || w <= 0 || ldz < C) return NNR_ERR_ARG;
  if (!kcnn_dims_ok(L, 1, w)) return NNR_ERR_UNSUPPORTED;
  if (n == 0) return NNR_OK;
  const long total = (long)n * C;
  hipLaunchKernelGGL(window_max_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, z, ldz, bias, total, C, L + w - 1, L - w + 1,
                     out, arg);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" size_t nnr_window_max_bwd_ws_floats(int n, int C) {
  return (n <= 0 || C <= 0) ? 0 : (size_t)((n + WM_TITLES - 1) / WM_TITLES) * (size_t)C;
}

extern "C" int nnr_window_max_bwd(const float* g, const uint8_t* arg, int n, int C, int L, int w, int lead_rows, float* dz, float* db, float* ws,
                                  hipStream_t stream) {
  if (!g || !arg || !dz || !db || !ws || n < 0 || C <= 0 || L <= 0 || w <= 0 || lead_rows < 0) return NNR_ERR_ARG;
  if (!kcnn_dims_ok(L, 1, w)) return NNR_ERR_UNSUPPORTED;
  const int groups = (n + WM_TITLES - 1) / WM_TITLES;
  if (n > 0) {
    const long total = (long)groups * C;
    hipLaunchKernelGGL(window_max_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, g, arg, n, C, L + w - 1, lead_rows, dz, ws);
    NNR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(partial_rows_sum_kernel<false>, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, (const float*)ws, groups, (long)C, db);   // plain store: the caller owns db
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
