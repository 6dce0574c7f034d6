// Deterministic embedding-row gradient (nn.Embedding backward, newsEncoders.py:117-118 under autograd; config.py:125-130 asks for
// reproducible runs): dtable[w, :] += sum over the token rows t with id w of mask(t, :) * dout[t, :].
//
// The f32-atomic scatter (misc.hip: embed_scatter_kernel) is bound by the memory-side atomic units (~1.3 TB/s chip-wide, 14x slower on
// hot rows) and adds a word's rows in whatever order the waves arrive.  Here the token rows are SORTED BY WORD ID once per step --
// the ids are known as soon as the token stream is planned, so the sort runs on the leaf stream under the forward pass, off the
// critical chain -- and the backward pass is a segmented reduction over the sorted list:
//   * nnr_token_sort: keys = word id of each live packed row (rows beyond the live count / invalid ids -> the pad key V), values =
//     row index; stable LSD radix sort (rocPRIM's device radix sort, compiled into this library from its headers), only the
//     ceil(log2(V + 1)) significant bits.  Stable => inside a word's segment the rows stay in ascending row order.
//   * nnr_embed_scatter_sorted: the segmented reduction of csrc/sorted_rows.h over the sorted rows (chunks of 32, 8 gradient rows in
//     flight in both passes), an occurrence being a packed token row and its addend mask(row, col) * dout[row, col].  The table gradient
//     receives one such call per token stream and step, so the table row is written with atomics (sorted_rows.h: ATOMIC).
#include <cstring>
#include <string.h>
#include "sorted_rows.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int SS_CH = 32;        // sorted rows per wave
constexpr int SS_MAXJ = 5;       // columns per lane: dim <= 320
constexpr int SS_FL = 8;         // rows in flight per wave, both passes

__global__ __launch_bounds__(256) void token_sort_keys_kernel(const int* __restrict__ tok, long cap, const int* __restrict__ n_dev, unsigned V,
                                                              unsigned* __restrict__ keys, int* __restrict__ rows) {
  const long n = n_dev ? min(cap, (long)*n_dev) : cap;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < cap; i += (long)gridDim.x * blockDim.x) {
    unsigned k = V;
    if (i < n) {
      const int t = tok[i];
      if (t >= 0 && (unsigned)t < V) k = (unsigned)t;
    }
    keys[i] = k;
    rows[i] = (int)i;
  }
}

// sorted_rows.h functor: a sorted entry is a row of dout; it adds the row under the dropout mask of the forward gather
struct ScatterRows {
  struct Rec { int row; };
  static constexpr int NV = 1;
  const float* dout;
  const int* rows;
  int dim;
  uint32_t seed, thr;
  float scale;
  __device__ Rec pad() const { return {0}; }
  __device__ Rec record(long p, bool) const { return {rows[p]}; }
  __device__ int nv() const { return 1; }
  __device__ const Rec& prep(const Rec& r) const { return r; }
  __device__ const float* row(const Rec& r, int) const { return dout + (long)r.row * dim; }
  __device__ float addend(const Rec& r, int col, bool in, const float (&v)[1]) const {
    float x = in ? v[0] : 0.f;
    if (thr) x = nnr_keep(seed, (uint64_t)r.row * dim + col, thr) ? x * scale : 0.f;
    return x;
  }
};

__global__ __launch_bounds__(256) void embed_scatter_sorted_kernel(const float* __restrict__ dout, const unsigned* __restrict__ keys,
                                                                   const int* __restrict__ rows, long cap, unsigned V, int dim,
                                                                   float* __restrict__ dtable, uint32_t seed, uint32_t thr, float scale,
                                                                   float* __restrict__ partial) {
  sorted_rows::pass1<SS_CH, SS_MAXJ, SS_FL, true, false>(ScatterRows{dout, rows, dim, seed, thr, scale}, keys, cap, V, dim, dtable, partial);
}

__global__ __launch_bounds__(256) void embed_scatter_sorted_fix_kernel(const unsigned* __restrict__ keys, long cap, unsigned V, int dim,
                                                                       float* __restrict__ dtable, const float* __restrict__ partial) {
  sorted_rows::fix<SS_CH, SS_MAXJ, SS_FL, true>(keys, cap, V, dim, dtable, partial);
}

int key_bits(unsigned V) {
  int b = 1;
  while (b < 32 && (V >> b)) ++b;
  return b;
}

}  // namespace

extern "C" size_t nnr_token_sort_workspace_bytes(long cap, int vocab) {
  if (cap <= 0 || vocab <= 0) return 0;
  size_t bytes = 0;
  unsigned* k = nullptr;
  int* r = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, r, r, (size_t)cap, 0u, (unsigned)key_bits((unsigned)vocab), (hipStream_t)0) != hipSuccess) return 0;
  return bytes + 256;
}

extern "C" int nnr_token_sort(const int* tok, long cap, const int* n_dev, int vocab, unsigned* keys_tmp, int* rows_tmp, unsigned* keys_sorted,
                              int* rows_sorted, void* temp, size_t temp_bytes, hipStream_t stream) {
  if (!tok || !keys_tmp || !rows_tmp || !keys_sorted || !rows_sorted || !temp || cap < 0 || vocab <= 0) return NNR_ERR_ARG;
  if (cap == 0) return NNR_OK;
  const int blocks = (int)((cap + 255) / 256 > 2048 ? 2048 : (cap + 255) / 256);
  hipLaunchKernelGGL(token_sort_keys_kernel, dim3(blocks), dim3(256), 0, stream, tok, cap, n_dev, (unsigned)vocab, keys_tmp, rows_tmp);
  NNR_CHECK_LAUNCH();
  size_t need = 0;
  if (rocprim::radix_sort_pairs(nullptr, need, keys_tmp, keys_sorted, rows_tmp, rows_sorted, (size_t)cap, 0u, (unsigned)key_bits((unsigned)vocab), stream) != hipSuccess)
    return NNR_ERR_LAUNCH;
  if (need > temp_bytes) return NNR_ERR_ARG;
  if (rocprim::radix_sort_pairs(temp, need, keys_tmp, keys_sorted, rows_tmp, rows_sorted, (size_t)cap, 0u, (unsigned)key_bits((unsigned)vocab), stream) != hipSuccess)
    return NNR_ERR_LAUNCH;
  return NNR_OK;
}

extern "C" size_t nnr_embed_scatter_sorted_workspace_floats(long cap) {
  return sorted_rows::ws_floats(cap, SS_CH, SS_MAXJ);
}

extern "C" int nnr_embed_scatter_sorted(const float* dout, const unsigned* keys_sorted, const int* rows_sorted, long cap, int vocab, int dim,
                                        float* dtable, float p, uint32_t seed, float* partial_ws, hipStream_t stream) {
  if (!dout || !keys_sorted || !rows_sorted || !dtable || !partial_ws || cap < 0 || vocab <= 0 || dim <= 0 || dim > 64 * SS_MAXJ) return NNR_ERR_ARG;
  if (cap == 0) return NNR_OK;
  const uint32_t thr = nnr_drop_thresh(p);
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const unsigned blocks = sorted_rows::blocks(cap, SS_CH);
  hipLaunchKernelGGL(embed_scatter_sorted_kernel, dim3(blocks), dim3(256), 0, stream, dout, keys_sorted, rows_sorted, cap, (unsigned)vocab, dim, dtable,
                     seed, thr, scale, partial_ws);
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(embed_scatter_sorted_fix_kernel, dim3(blocks), dim3(256), 0, stream, keys_sorted, cap, (unsigned)vocab, dim, dtable, partial_ws);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
