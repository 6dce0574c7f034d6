// NAML family (variantEncoders.py:102-187 NAML_Title / NAML_Content): the multi-view attention that closes the encoder,
//   rep[i] = sum over the views v of softmax_v(score_v[i]) * row_v[i],   score = affine2 . tanh(affine1(row)).
//
// A news has Vt text views (1 here, 2 for NAML proper) whose rows [n, C] and scores [n] are per news, and two TABLE views -- category and
// subCategory -- whose row is a pure function of an id: relu(affine(embedding table)) has R rows (18 and 285 at MIND sizes) whatever the
// number of news, so rows and scores of the table views are computed once per table row by the GEMM family and only indexed here.
//   * view_pool_fwd_kernel: one wave per news: gathers the V = Vt + 2 scores, softmax with the maximum subtracted, alpha [n, V] (view order:
//     text views, category, subCategory) and the weighted sum of the V rows.  The [n, V, C] stack of the reference never exists.
//   * view_pool_bwd_news_kernel: one wave per news: dalpha_v = <dout, row_v>, ds_v = alpha_v (dalpha_v - sum_u alpha_u dalpha_u); the text
//     views' dense gradient rows alpha_v dout and their ds; the table views' ds into a [2, n] workspace.
//   * view_pool_bwd_table_kernel: the table views' gradients are sums over the news that share an id.  One workgroup per (table row, chunk
//     of 64 columns): its four waves take the four consecutive quarters of the news list, each scans its quarter's ids 64 at a time (one
//     ballot: the ids are 14 KB at batch 64 and stay in L2), walks the matches in ascending order with eight rows in flight, and the four
//     partial sums are added in wave order -- no sort, no float atomics, no communication between workgroups, same inputs -> same bits.
//     A table row no news uses gets zeros WRITTEN.  Every loop is bounded by a host argument (n, C) or by a constant.
//     (A first version walked the news sorted by id through csrc/sort.hip: the two sorts cost the step more launches than the view
//     attention has left -- these encoder pairs are bound by the host's enqueue rate --, see profiles/naml_summary.md.)
// An id outside [0, R) reads table row 0 and sends no gradient (no table row matches it).
//
// The text stream's convolution Conv1d(E -> C, window k odd, padding (k - 1) / 2) is ONE product on the GEMM family (csrc/gemm.hip, untouched)
// once its A operand is the halo-padded image Xp[n][Lp = L + k - 1][E] ((k - 1) / 2 leading and trailing zero rows per news): the window of
// output position t is the contiguous k E floats from padded row t on (lda = E < K = k E, as csrc/kcnn.hip does for the 2-D convolution).
// The product's epilogue writes the live rows compact through its row map (row i Lp + t -> i L + t, rows t >= L dropped): everything behind
// the convolution keeps its [n L, C] layout.
//   * conv1d_image_fwd_kernel: one wave per padded row: dropout(word_table[text[i, t]]) or a zero halo row, in ONE pass.  The keep-mask is
//     keyed on the COMPACT index (i L + t) E + e: the mask nnr_embed_gather draws for the same seed on the un-padded rows.
//   * conv1d_dz_pad_kernel: the backward's A operand dz[(k - 1) + n Lp][C]: relu backward of the compact gradient at the live rows, zeros in
//     the k - 1 leading rows and at every row t >= L -- those zeros keep one news's gradient out of its neighbour's rows.  The data gradient
//     is then one product against the transposed, window-reversed weight, the weight gradient one TN product over the overlapping rows.
//   * conv1d_image_bwd_kernel: the word rows' gradient compact again, through the word rows' keep-mask (same key as forward).
#include "common.h"

namespace {

constexpr int VP_FL = 8;          // rows in flight per wave in the segmented reduction
constexpr int VP_COLS = 64;       // columns per workgroup of the segmented reduction

__device__ __forceinline__ int vp_row(const int* __restrict__ ids, long i, int R) {
  const int r = ids[i];
  return (r >= 0 && r < R) ? r : 0;
}

__global__ __launch_bounds__(256) void view_pool_fwd_kernel(const float* __restrict__ t0, const float* __restrict__ ts0, const float* __restrict__ t1,
                                                            const float* __restrict__ ts1, const float* __restrict__ rowsA,
                                                            const float* __restrict__ scoreA, const int* __restrict__ idsA, int Ra,
                                                            const float* __restrict__ rowsB, const float* __restrict__ scoreB,
                                                            const int* __restrict__ idsB, int Rb, int n, int C, float* __restrict__ alpha,
                                                            float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long i = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (i >= n) return;
  const bool two = t1 != nullptr;
  const int V = two ? 4 : 3;
  const int ra = vp_row(idsA, i, Ra), rb = vp_row(idsB, i, Rb);
  const float s0 = ts0[i], s1 = two ? ts1[i] : -INFINITY, sa = scoreA[ra], sb = scoreB[rb];
  const float m = fmaxf(fmaxf(s0, s1), fmaxf(sa, sb));
  const float e0 = expf(s0 - m), e1 = two ? expf(s1 - m) : 0.f, ea = expf(sa - m), eb = expf(sb - m);
  const float inv = 1.f / (((e0 + e1) + ea) + eb);
  const float a0 = e0 * inv, a1 = e1 * inv, aa = ea * inv, ab = eb * inv;
  if (lane == 0) {
    float* __restrict__ al = alpha + i * V;
    al[0] = a0;
    if (two) al[1] = a1;
    al[V - 2] = aa;
    al[V - 1] = ab;
  }
  const float* __restrict__ x0 = t0 + i * C;
  const float* __restrict__ x1 = two ? t1 + i * C : x0;
  const float* __restrict__ xa = rowsA + (long)ra * C;
  const float* __restrict__ xb = rowsB + (long)rb * C;
  float* __restrict__ o = out + i * C;
  for (int c = lane; c < C; c += 64) {
    float acc = a0 * x0[c];
    if (two) acc += a1 * x1[c];
    acc += aa * xa[c];
    acc += ab * xb[c];
    o[c] = acc;
  }
}

__global__ __launch_bounds__(256) void view_pool_bwd_news_kernel(const float* __restrict__ dout, const float* __restrict__ t0,
                                                                 const float* __restrict__ t1, const float* __restrict__ rowsA,
                                                                 const int* __restrict__ idsA, int Ra, const float* __restrict__ rowsB,
                                                                 const int* __restrict__ idsB, int Rb, const float* __restrict__ alpha, int n,
                                                                 int C, float* __restrict__ dt0, float* __restrict__ dts0, float* __restrict__ dt1,
                                                                 float* __restrict__ dts1, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const long i = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (i >= n) return;
  const bool two = t1 != nullptr;
  const int V = two ? 4 : 3;
  const int ra = vp_row(idsA, i, Ra), rb = vp_row(idsB, i, Rb);
  const float* __restrict__ g = dout + i * C;
  const float* __restrict__ x0 = t0 + i * C;
  const float* __restrict__ x1 = two ? t1 + i * C : x0;
  const float* __restrict__ xa = rowsA + (long)ra * C;
  const float* __restrict__ xb = rowsB + (long)rb * C;
  const float* __restrict__ al = alpha + i * V;
  const float a0 = al[0], a1 = two ? al[1] : 0.f, aa = al[V - 2], ab = al[V - 1];
  float d0 = 0.f, d1 = 0.f, da = 0.f, db = 0.f;
  float* __restrict__ o0 = dt0 + i * C;
  float* __restrict__ o1 = two ? dt1 + i * C : nullptr;
  for (int c = lane; c < C; c += 64) {
    const float gv = g[c];
    d0 += gv * x0[c];
    if (two) d1 += gv * x1[c];
    da += gv * xa[c];
    db += gv * xb[c];
    o0[c] = a0 * gv;
    if (two) o1[c] = a1 * gv;
  }
  d0 = wave_sum(d0);
  d1 = wave_sum(d1);
  da = wave_sum(da);
  db = wave_sum(db);
  const float dot = ((a0 * d0 + a1 * d1) + aa * da) + ab * db;
  if (lane == 0) {
    dts0[i] = a0 * (d0 - dot);
    if (two) dts1[i] = a1 * (d1 - dot);
    ws[i] = aa * (da - dot);
    ws[(long)n + i] = ab * (db - dot);
  }
}

__global__ __launch_bounds__(256) void view_pool_bwd_table_kernel(const float* __restrict__ dout, const float* __restrict__ alpha, int V,
                                                                  const float* __restrict__ ws, int n, int C, int Ra, int Rb,
                                                                  const int* __restrict__ idsA, const int* __restrict__ idsB,
                                                                  float* __restrict__ drowsA, float* __restrict__ dscoreA,
                                                                  float* __restrict__ drowsB, float* __restrict__ dscoreB) {
  __shared__ float red[4][VP_COLS];
  __shared__ float sred[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool second = (int)blockIdx.x >= Ra;                      // (uniform over the workgroup)
  const int r = second ? (int)blockIdx.x - Ra : (int)blockIdx.x;
  const int* __restrict__ ids = second ? idsB : idsA;
  const float* __restrict__ ds = ws + (second ? (long)n : 0L);
  const int vcol = V - 2 + (second ? 1 : 0);
  const int quarter = (n + 3) / 4;
  const int w0 = min(n, wv * quarter), w1 = min(n, w0 + quarter);
  const int col = blockIdx.y * VP_COLS + lane;
  const int colc = min(col, C - 1);
  const bool want_score = blockIdx.y == 0;
  float acc = 0.f, sacc = 0.f;
  for (int base = w0; base < w1; base += 64) {
    const int j = base + lane;
    unsigned long long m = __ballot(j < w1 && ids[min(j, w1 - 1)] == r);      // the news of these 64 that name row r, ascending
    for (int it = 0; it < 64 / VP_FL && m; ++it) {
      // VP_FL rows in flight: every load is issued before any is used; slots past the last match re-read news `base` and are dropped below
      int iu[VP_FL];
      bool ok[VP_FL];
#pragma unroll
      for (int u = 0; u < VP_FL; ++u) {
        ok[u] = m != 0ull;
        iu[u] = ok[u] ? base + __builtin_ctzll(m) : base;
        m &= m - 1ull;                                                        // (0 stays 0)
      }
      float a[VP_FL], g[VP_FL], d[VP_FL];
#pragma unroll
      for (int u = 0; u < VP_FL; ++u) {
        a[u] = alpha[(long)iu[u] * V + vcol];
        g[u] = dout[(long)iu[u] * C + colc];
        d[u] = want_score ? ds[iu[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < VP_FL; ++u)
        if (ok[u]) { acc += a[u] * g[u]; sacc += d[u]; }
    }
  }
  red[wv][lane] = acc;
  if (lane == 0) sred[wv] = sacc;
  __syncthreads();
  if (wv == 0) {
    if (col < C) (second ? drowsB : drowsA)[(long)r * C + col] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    if (want_score && lane == 0) (second ? dscoreB : dscoreA)[r] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
  }
}

// ---------------------------------------------------------------------------------------------- padded-row convolution image
constexpr int C1_MAX_K = 8;

static inline bool conv1d_dims_ok(int n, int L, int W, int k) { return n > 0 && L > 0 && W > 0 && k > 0 && (k & 1) && k <= C1_MAX_K; }

// one wave per padded row; VEC = 4: float4 accesses (E % 4 == 0, 16-byte aligned bases), VEC = 1: scalar
template <int VEC>
__global__ __launch_bounds__(256) void conv1d_image_fwd_kernel(const float* __restrict__ table, int V, const int* __restrict__ text, long rows, int L,
                                                               int E, int k, uint32_t seed, uint32_t thr, float scale, float* __restrict__ Xp) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int Lp = L + k - 1, pad = (k - 1) / 2;
  const long i = r / Lp;
  const int t = (int)(r - i * Lp) - pad;
  float* __restrict__ dst = Xp + r * (long)E;
  const long tok = i * L + t;
  int id = -1;
  if (t >= 0 && t < L) id = text[tok];
  const bool live = id >= 0 && id < V;
  const float* __restrict__ src = table + (long)(live ? id : 0) * E;
  if (VEC == 4) {
    for (int q = lane; q < E / 4; q += 64) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        v = reinterpret_cast<const f32x4*>(src)[q];
        if (thr) {
          bool kp[4];
          nnr_keep4(seed, (uint64_t)tok * E + 4 * q, thr, kp);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = kp[e] ? v[e] * scale : 0.f;
        }
      }
      reinterpret_cast<f32x4*>(dst)[q] = v;
    }
  } else {
    for (int q = lane; q < E; q += 64) {
      float v = 0.f;
      if (live) {
        v = src[q];
        if (thr) v = nnr_keep(seed, (uint64_t)tok * E + q, thr) ? v * scale : 0.f;
      }
      dst[q] = v;
    }
  }
}

// one wave per row of dz[(k - 1) + n Lp][C]
template <int VEC>
__global__ __launch_bounds__(256) void conv1d_dz_pad_kernel(const float* __restrict__ dy, const float* __restrict__ y, long rows, int L, int C, int k,
                                                            float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int Lp = L + k - 1, lead = k - 1;
  float* __restrict__ dst = dz + r * (long)C;
  const long rr = r - lead;
  const long i = rr >= 0 ? rr / Lp : 0;
  const int t = rr >= 0 ? (int)(rr - i * Lp) : L;
  const bool live = t < L;
  const long src = (i * L + (live ? t : 0)) * (long)C;
  if (VEC == 4) {
    for (int q = lane; q < C / 4; q += 64) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        const f32x4 g = reinterpret_cast<const f32x4*>(dy + src)[q], a = reinterpret_cast<const f32x4*>(y + src)[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = a[e] > 0.f ? g[e] : 0.f;
      }
      reinterpret_cast<f32x4*>(dst)[q] = v;
    }
  } else {
    for (int q = lane; q < C; q += 64) dst[q] = (live && y[src + q] > 0.f) ? dy[src + q] : 0.f;
  }
}

// one wave per word row (i, t): dx = keep-mask * dXp at the row's place in the image; halo rows are not read
template <int VEC>
__global__ __launch_bounds__(256) void conv1d_image_bwd_kernel(const float* __restrict__ dXp, long rows, int L, int E, int k, uint32_t seed,
                                                               uint32_t thr, float scale, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);        // r = i * L + t
  if (r >= rows) return;
  const int Lp = L + k - 1, pad = (k - 1) / 2;
  const long i = r / L;
  const float* __restrict__ g = dXp + (i * Lp + (r - i * L) + pad) * (long)E;
  float* __restrict__ o = dx + r * (long)E;
  if (VEC == 4) {
    for (int q = lane; q < E / 4; q += 64) {
      f32x4 v = reinterpret_cast<const f32x4*>(g)[q];
      if (thr) {
        bool kp[4];
        nnr_keep4(seed, (uint64_t)r * E + 4 * q, thr, kp);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = kp[e] ? v[e] * scale : 0.f;
      }
      reinterpret_cast<f32x4*>(o)[q] = v;
    }
  } else {
    for (int q = lane; q < E; q += 64) {
      float v = g[q];
      if (thr) v = nnr_keep(seed, (uint64_t)r * E + q, thr) ? v * scale : 0.f;
      o[q] = v;
    }
  }
}

}  // namespace

extern "C" int nnr_view_pool_fwd(const float* t0, const float* ts0, const float* t1, const float* ts1, int Vt, const float* rowsA,
                                 const float* scoreA, const int* idsA, int Ra, const float* rowsB, const float* scoreB, const int* idsB, int Rb,
                                 int n, int C, float* alpha, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || Ra <= 0 || Rb <= 0 || Vt < 1 || Vt > 2) return NNR_ERR_UNSUPPORTED;
  if (!t0 || !ts0 || !rowsA || !scoreA || !idsA || !rowsB || !scoreB || !idsB || !alpha || !out) return NNR_ERR_ARG;
  if (Vt == 2 && (!t1 || !ts1)) return NNR_ERR_ARG;
  hipLaunchKernelGGL(view_pool_fwd_kernel, dim3((unsigned)((n + 3L) / 4)), dim3(256), 0, stream, t0, ts0, Vt == 2 ? t1 : nullptr,
                     Vt == 2 ? ts1 : nullptr, rowsA, scoreA, idsA, Ra, rowsB, scoreB, idsB, Rb, n, C, alpha, out);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_view_pool_bwd(const float* dout, const float* t0, const float* t1, int Vt, const float* rowsA, const int* idsA, int Ra,
                                 const float* rowsB, const int* idsB, int Rb, const float* alpha, int n, int C, float* dt0, float* dts0,
                                 float* dt1, float* dts1, float* drowsA, float* dscoreA, float* drowsB, float* dscoreB, float* ws,
                                 hipStream_t stream) {
  if (n <= 0 || C <= 0 || Ra <= 0 || Rb <= 0 || Vt < 1 || Vt > 2) return NNR_ERR_UNSUPPORTED;
  if (!dout || !t0 || !rowsA || !idsA || !rowsB || !idsB || !alpha || !dt0 || !dts0 || !drowsA ||
      !dscoreA || !drowsB || !dscoreB || !ws)
    return NNR_ERR_ARG;
  if (Vt == 2 && (!t1 || !dt1 || !dts1)) return NNR_ERR_ARG;
  hipLaunchKernelGGL(view_pool_bwd_news_kernel, dim3((unsigned)((n + 3L) / 4)), dim3(256), 0, stream, dout, t0, Vt == 2 ? t1 : nullptr, rowsA, idsA,
                     Ra, rowsB, idsB, Rb, alpha, n, C, dt0, dts0, dt1, dts1, ws);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(view_pool_bwd_table_kernel, dim3((unsigned)(Ra + Rb), (unsigned)((C + VP_COLS - 1) / VP_COLS)), dim3(256), 0, stream, dout, alpha,
                     Vt + 2, (const float*)ws, n, C, Ra, Rb, idsA, idsB, drowsA, dscoreA, drowsB, dscoreB);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_conv1d_image_fwd(const float* word_table, int V, const int* text, int n, int L, int E, int k, float p, uint32_t seed, float* Xp,
                                    hipStream_t stream) {
  if (!conv1d_dims_ok(n, L, E, k) || V <= 0) return NNR_ERR_UNSUPPORTED;
  if (!word_table || !text || !Xp) return NNR_ERR_ARG;
  const uint32_t thr = nnr_drop_thresh(p);
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const long rows = (long)n * (L + k - 1);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (E % 4 == 0 && al16(word_table) && al16(Xp))
    hipLaunchKernelGGL(conv1d_image_fwd_kernel<4>, grid, dim3(256), 0, stream, word_table, V, text, rows, L, E, k, seed, thr, scale, Xp);
  else
    hipLaunchKernelGGL(conv1d_image_fwd_kernel<1>, grid, dim3(256), 0, stream, word_table, V, text, rows, L, E, k, seed, thr, scale, Xp);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_conv1d_dz_pad(const float* dy, const float* y, int n, int L, int C, int k, float* dz, hipStream_t stream) {
  if (!conv1d_dims_ok(n, L, C, k)) return NNR_ERR_UNSUPPORTED;
  if (!dy || !y || !dz) return NNR_ERR_ARG;
  const long rows = (long)(k - 1) + (long)n * (L + k - 1);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (C % 4 == 0 && al16(dy) && al16(y) && al16(dz))
    hipLaunchKernelGGL(conv1d_dz_pad_kernel<4>, grid, dim3(256), 0, stream, dy, y, rows, L, C, k, dz);
  else
    hipLaunchKernelGGL(conv1d_dz_pad_kernel<1>, grid, dim3(256), 0, stream, dy, y, rows, L, C, k, dz);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_conv1d_image_bwd(const float* dXp, int n, int L, int E, int k, float p, uint32_t seed, float* dx, hipStream_t stream) {
  if (!conv1d_dims_ok(n, L, E, k)) return NNR_ERR_UNSUPPORTED;
  if (!dXp || !dx) return NNR_ERR_ARG;
  const uint32_t thr = nnr_drop_thresh(p);
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const long rows = (long)n * L;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (E % 4 == 0 && al16(dXp) && al16(dx))
    hipLaunchKernelGGL(conv1d_image_bwd_kernel<4>, grid, dim3(256), 0, stream, dXp, rows, L, E, k, seed, thr, scale, dx);
  else
    hipLaunchKernelGGL(conv1d_image_bwd_kernel<1>, grid, dim3(256), 0, stream, dXp, rows, L, E, k, seed, thr, scale, dx);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
