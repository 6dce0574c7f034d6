// Shared device helpers for libnnr_hip (gfx950 / CDNA4 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nnr_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define NNR_CHECK_LAUNCH()                                   \
  do {                                                       \
    hipError_t e_ = hipGetLastError();                       \
    if (e_ != hipSuccess) return NNR_ERR_LAUNCH;             \
  } while (0)

// ---------------------------------------------------------------- counter-based dropout
// keep(idx) is a pure function of (seed, idx): forward and backward recompute the same mask,
// nothing is stored.  lowbias32 finaliser (two rounds) -- statistical quality is ample for dropout.
__device__ __forceinline__ uint32_t nnr_hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
// One 32-bit hash serves TWO neighbouring elements (16 bits each): keep(idx) tests bits [16*(idx&1), +16) of hash(idx>>1)
// against a 16-bit threshold, so P(drop) is p rounded to 1/65536 and a float4 of elements costs two hashes.
__device__ __forceinline__ uint32_t nnr_hash_pair(uint32_t seed, uint64_t pair) {
  return nnr_hash32((uint32_t)pair ^ nnr_hash32((uint32_t)(pair >> 32) + seed));
}
__device__ __forceinline__ bool nnr_keep(uint32_t seed, uint64_t idx, uint32_t thresh) {
  const uint32_t h = nnr_hash_pair(seed, idx >> 1);
  return ((h >> (16u * (uint32_t)(idx & 1))) & 0xFFFFu) >= thresh;   // P(keep) = 1 - thresh / 65536
}
// four consecutive elements starting at an index that is a multiple of 4 (the common float4 case): two hashes
__device__ __forceinline__ void nnr_keep4(uint32_t seed, uint64_t idx4, uint32_t thresh, bool (&k)[4]) {
  const uint32_t h0 = nnr_hash_pair(seed, idx4 >> 1), h1 = nnr_hash_pair(seed, (idx4 >> 1) + 1);
  k[0] = (h0 & 0xFFFFu) >= thresh; k[1] = (h0 >> 16) >= thresh; k[2] = (h1 & 0xFFFFu) >= thresh; k[3] = (h1 >> 16) >= thresh;
}
static inline uint32_t nnr_drop_thresh(float p) {
  if (p <= 0.f) return 0u;
  double t = (double)p * 65536.0 + 0.5;
  if (t > 65535.0) t = 65535.0;
  return (uint32_t)t;
}

// ---------------------------------------------------------------- wave-level reductions (64 lanes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// sum over the 16 lanes that share (lane >> 4)
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Hardware-transcendental activations for the LSTM cell update, which sits on the critical path of the recurrence
// (128 dependent steps): v_exp_f32 + v_rcp_f32, ~4 instructions instead of the ~40-60 of OCML expf / tanhf / division.
// Absolute error ~2e-7 (1-2 ulp of the result), far inside the 1e-4 parity bar (tests/test_hip_ops_gpu.py: 2e-5).
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 2.f * fast_sigmoid(2.f * x) - 1.f; }

// ---------------------------------------------------------------- V = 4 (float4) / V = 1 (scalar) variants of one kernel body
template <int V> struct vec_t;
template <> struct vec_t<4> { typedef f32x4 type; };
template <> struct vec_t<1> { typedef float type; };
template <int V> __device__ __forceinline__ typename vec_t<V>::type vzero();
template <> __device__ __forceinline__ f32x4 vzero<4>() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
template <> __device__ __forceinline__ float vzero<1>() { return 0.f; }
__device__ __forceinline__ float vdot(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }
__device__ __forceinline__ float vdot(float a, float b) { return a * b; }
__device__ __forceinline__ f32x4 vtanh(f32x4 z) { return f32x4{tanhf(z[0]), tanhf(z[1]), tanhf(z[2]), tanhf(z[3])}; }
__device__ __forceinline__ float vtanh(float z) { return tanhf(z); }

// ---------------------------------------------------------------- row loads of the width a row's alignment allows (float4 / float2 / float)
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

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// blocks of 256 threads for an element-wise kernel with a grid-stride loop over `total` elements, capped
static inline unsigned grid_for(long total, long cap = 8192) {
  const long b = (total + 255) / 256;
  return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

// ---------------------------------------------------------------- fixed-order sum of partial rows
// sum over q = 0 .. rows - 1, ascending, of ws[q * stride + p]: strictly sequential adds (same inputs -> same bits), four loads in flight
__device__ __forceinline__ float partial_rows_sum(const float* __restrict__ ws, int rows, long stride, long p) {
  float t = 0.f;
  int q = 0;
  for (; q + 4 <= rows; q += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ws[(long)(q + u) * stride + p];
#pragma unroll
    for (int u = 0; u < 4; ++u) t += v[u];
  }
  for (; q < rows; ++q) t += ws[(long)q * stride + p];
  return t;
}
// out[p] (+)= the partial rows ws[rows][n] in row order, one thread per element
template <bool ACCUMULATE>
__global__ __launch_bounds__(256) void partial_rows_sum_kernel(const float* __restrict__ ws, int rows, long n, float* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float t = partial_rows_sum(ws, rows, n, p);
  out[p] = ACCUMULATE ? out[p] + t : t;
}
