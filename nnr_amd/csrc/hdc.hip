// HDC news encoder (newsEncoders.py:244-278): the bandwidth kernels around its dilated convolutions, which run on the GEMM family.
//
// Activations are position-major: a news is S = max_title_length + 2 rows (category row, subCategory row, title word rows) of C floats.
// A dilated Conv1d(window 3, dilation d, padding d) over such rows is three accumulating products of csrc/gemm.hip (untouched) once its
// input has d zero halo rows on both sides of every news: tap k reads the same padded buffer shifted by k d rows.  So every layer's input
// exists twice: compact [n][S][C] (what the matching images of the FIM user encoder read) and padded [n][S + 2 d][C].
// The kernels here build the first pair from the three tables, apply LayerNorm([F, S]) + ReLU per news (mean and variance over all F S
// values, affine parameters [F, S] read in place: index f S + s), and do its backward.  They move bytes: no MFMA.
#include "common.h"

namespace {

constexpr int LN_CHUNK = 32;          // news per partial sum of the affine-parameter gradients

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// one wave per padded row (i, q): halo rows zero; row s = q - pad of news i comes from the category table (s = 0), the subCategory table
// (s = 1) or the word table (s >= 2); written to the padded and to the compact buffer.  tok_* [n S]: the id at the rows of each table, -1 elsewhere.
__global__ __launch_bounds__(256) void hdc_seq_fwd_kernel(const float* __restrict__ word, int V, const float* __restrict__ cat_t, int ncat,
                                                          const float* __restrict__ sub_t, int nsub, const int* __restrict__ text,
                                                          const int* __restrict__ cat, const int* __restrict__ sub, long rows, int L, int E, int pad,
                                                          float* __restrict__ d0, float* __restrict__ d0p, int* __restrict__ tok_w,
                                                          int* __restrict__ tok_c, int* __restrict__ tok_s) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int S = L + 2, Sp = S + 2 * pad;
  const long i = r / Sp;
  const int s = (int)(r - i * Sp) - pad;
  float* __restrict__ dp = d0p + r * E;
  if (s < 0 || s >= S) {
    for (int q = lane; q < E; q += 64) dp[q] = 0.f;
    return;
  }
  const float* src = nullptr;
  int id, tw = -1, tc = -1, ts = -1;
  if (s == 0) { id = cat[i]; if (id >= 0 && id < ncat) { src = cat_t + (long)id * E; tc = id; } }
  else if (s == 1) { id = sub[i]; if (id >= 0 && id < nsub) { src = sub_t + (long)id * E; ts = id; } }
  else { id = text[i * L + s - 2]; if (id >= 0 && id < V) { src = word + (long)id * E; tw = id; } }
  float* __restrict__ dc = d0 + (i * S + s) * E;
  for (int q = lane; q < E; q += 64) {
    const float v = src ? src[q] : 0.f;
    dp[q] = v;
    dc[q] = v;
  }
  if (lane == 0) { tok_w[i * S + s] = tw; tok_c[i * S + s] = tc; tok_s[i * S + s] = ts; }
}

// one workgroup per news: z rows [0, S) of the news' Spz rows -> y compact, and (optional) yp padded with `pad` zero halo rows
__global__ __launch_bounds__(256) void hdc_ln_relu_fwd_kernel(const float* __restrict__ z, int Spz, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int S, int F, float eps, float* __restrict__ y,
                                                              float* __restrict__ yp, int pad, float* __restrict__ stats) {
  __shared__ float red[4];
  const long i = blockIdx.x;
  const int n = S * F;
  const float* __restrict__ zi = z + i * (long)Spz * F;
  float s = 0.f;
  for (int e = threadIdx.x; e < n; e += 256) s += zi[e];
  const float mean = block_sum(s, red) / (float)n;
  float q = 0.f;
  for (int e = threadIdx.x; e < n; e += 256) { const float d = zi[e] - mean; q = __builtin_fmaf(d, d, q); }
  const float rstd = 1.f / sqrtf(block_sum(q, red) / (float)n + eps);
  if (threadIdx.x == 0) { stats[2 * i] = mean; stats[2 * i + 1] = rstd; }
  float* __restrict__ yi = y + i * (long)n;
  float* __restrict__ ypi = yp ? yp + i * (long)(S + 2 * pad) * F : nullptr;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int sp = e / F, f = e - sp * F;
    const float v = fmaxf((zi[e] - mean) * rstd * gamma[f * S + sp] + beta[f * S + sp], 0.f);
    yi[e] = v;
    if (ypi) ypi[pad * F + e] = v;
  }
  if (ypi)
    for (int e = threadIdx.x; e < pad * F; e += 256) { ypi[e] = 0.f; ypi[(pad + S) * F + e] = 0.f; }
}

// partial affine-parameter gradients of LN_CHUNK news: ws[chunk][0][e] = sum dpre xhat, ws[chunk][1][e] = sum dpre (dpre = dy where y > 0)
__global__ __launch_bounds__(256) void hdc_ln_param_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z,
                                                           int Spz, const float* __restrict__ stats, int nnews, int S, int F,
                                                           float* __restrict__ ws) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n = S * F;
  if (e >= n) return;
  const int i0 = blockIdx.y * LN_CHUNK, i1 = min(nnews, i0 + LN_CHUNK);
  float g = 0.f, b = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float dp = y[(long)i * n + e] > 0.f ? dy[(long)i * n + e] : 0.f;
    const float xh = (z[(long)i * Spz * F + e] - stats[2 * i]) * stats[2 * i + 1];
    g = __builtin_fmaf(dp, xh, g);
    b += dp;
  }
  ws[((long)blockIdx.y * 2) * n + e] = g;
  ws[((long)blockIdx.y * 2 + 1) * n + e] = b;
}

__global__ __launch_bounds__(256) void hdc_ln_param_reduce_kernel(const float* __restrict__ ws, int chunks, int S, int F, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n = S * F;
  if (e >= n) return;
  const float g = partial_rows_sum(ws, chunks, 2L * n, e), b = partial_rows_sum(ws + n, chunks, 2L * n, e);
  const int sp = e / F, f = e - sp * F;
  dgamma[f * S + sp] += g;
  dbeta[f * S + sp] += b;
}

// one workgroup per news, IN PLACE: z rows [0, S) become dz, rows [S, Spz) become zero (what the shifted data-gradient products need)
__global__ __launch_bounds__(256) void hdc_ln_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ z, int Spz,
                                                              const float* __restrict__ stats, const float* __restrict__ gamma, int S, int F) {
  __shared__ float red[4];
  const long i = blockIdx.x;
  const int n = S * F;
  float* __restrict__ zi = z + i * (long)Spz * F;
  const float* __restrict__ dyi = dy + i * (long)n;
  const float* __restrict__ yi = y + i * (long)n;
  const float mean = stats[2 * i], rstd = stats[2 * i + 1];
  float s1 = 0.f, s2 = 0.f;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int sp = e / F, f = e - sp * F;
    const float dxh = yi[e] > 0.f ? dyi[e] * gamma[f * S + sp] : 0.f;
    s1 += dxh;
    s2 = __builtin_fmaf(dxh, (zi[e] - mean) * rstd, s2);
  }
  const float m1 = block_sum(s1, red) / (float)n;
  const float m2 = block_sum(s2, red) / (float)n;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int sp = e / F, f = e - sp * F;
    const float dxh = yi[e] > 0.f ? dyi[e] * gamma[f * S + sp] : 0.f;
    const float xh = (zi[e] - mean) * rstd;
    zi[e] = rstd * (dxh - m1 - xh * m2);
  }
  for (int e = n + threadIdx.x; e < Spz * F; e += 256) zi[e] = 0.f;
}

// out[i][s] = a[i][s] + bp[i][pad + s]  (a: compact or NULL, bp: padded with Sp rows per news); a first, then bp
__global__ __launch_bounds__(256) void hdc_unpad_add_kernel(const float* __restrict__ a, const float* __restrict__ bp, long total, int S, int Sp, int pad,
                                                            int C, float* __restrict__ out) {
  const long SC = (long)S * C;
  for (long o = blockIdx.x * 256L + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const long i = o / SC;
    const float v = bp[i * (long)Sp * C + (long)pad * C + (o - i * SC)];
    out[o] = a ? a[o] + v : v;
  }
}

}  // namespace

extern "C" int nnr_hdc_seq_fwd(const float* word_table, int V, const float* cat_table, int ncat, const float* sub_table, int nsub, const int* text,
                               const int* category, const int* subCategory, int n, int L, int E, int pad, float* d0, float* d0p, int* tok_word,
                               int* tok_cat, int* tok_sub, hipStream_t stream) {
  if (!word_table || !cat_table || !sub_table || !text || !category || !subCategory || !d0 || !d0p || !tok_word || !tok_cat || !tok_sub || V <= 0 ||
      ncat <= 0 || nsub <= 0 || n < 0 || L <= 0 || E <= 0 || pad < 0)
    return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  const long rows = (long)n * (L + 2 + 2 * pad);
  if ((rows + 3) / 4 > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(hdc_seq_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, word_table, V, cat_table, ncat, sub_table, nsub, text,
                     category, subCategory, rows, L, E, pad, d0, d0p, tok_word, tok_cat, tok_sub);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_hdc_ln_relu_fwd(const float* z, int z_rows, const float* gamma, const float* beta, int n, int S, int F, float eps, float* y,
                                   float* y_padded, int pad, float* stats, hipStream_t stream) {
  if (!z || !gamma || !beta || !y || !stats || n < 0 || S <= 0 || F <= 0 || z_rows < S || pad < 0) return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  hipLaunchKernelGGL(hdc_ln_relu_fwd_kernel, dim3((unsigned)n), dim3(256), 0, stream, z, z_rows, gamma, beta, S, F, eps, y, y_padded, pad, stats);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" size_t nnr_hdc_ln_bwd_ws_floats(int n, int S, int F) {
  return (n <= 0 || S <= 0 || F <= 0) ? 0 : (size_t)((n + LN_CHUNK - 1) / LN_CHUNK) * 2 * (size_t)S * F;
}

extern "C" int nnr_hdc_ln_relu_bwd(const float* dy, const float* y, float* z, int z_rows, const float* stats, const float* gamma, int n, int S, int F,
                                   float* dgamma_accum, float* dbeta_accum, float* ws, hipStream_t stream) {
  if (!dy || !y || !z || !stats || !gamma || !dgamma_accum || !dbeta_accum || !ws || n < 0 || S <= 0 || F <= 0 || z_rows < S) return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  const int chunks = (n + LN_CHUNK - 1) / LN_CHUNK, eb = (S * F + 255) / 256;
  if (chunks > 65535) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(hdc_ln_param_kernel, dim3((unsigned)eb, (unsigned)chunks), dim3(256), 0, stream, dy, y, (const float*)z, z_rows, stats, n, S, F, ws);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(hdc_ln_param_reduce_kernel, dim3((unsigned)eb), dim3(256), 0, stream, (const float*)ws, chunks, S, F, dgamma_accum, dbeta_accum);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(hdc_ln_relu_bwd_kernel, dim3((unsigned)n), dim3(256), 0, stream, dy, y, z, z_rows, stats, gamma, S, F);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_hdc_unpad_add(const float* a, const float* b_padded, int n, int S, int pad, int C, float* out, hipStream_t stream) {
  if (!b_padded || !out || n < 0 || S <= 0 || pad < 0 || C <= 0) return NNR_ERR_ARG;
  if (n == 0) return NNR_OK;
  const long total = (long)n * S * C;
  hipLaunchKernelGGL(hdc_unpad_add_kernel, dim3(grid_for(total)), dim3(256), 0, stream, a, b_padded, total, S, S + 2 * pad, pad, C, out);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
