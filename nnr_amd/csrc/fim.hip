// FIM user encoder (userEncoders.py:224-262): Conv3d + bias + ELU + MaxPool3d as ONE kernel family, forward and backward.
//
// The dense convolution output never exists in memory.  A workgroup owns one slab of pool cells (one image, one pooled depth, PHB pooled
// rows): it stages the slab's input footprint and the repacked weights in LDS, computes the P^3 convolution positions of every cell with
// fp32 FMAs in ONE fixed order (ci, kd, kh, kw -- so positions whose windows hold the same values give the same bits), and keeps per
// (cell, filter) the maximum and its one-byte index in the window's (depth, row, column) scan order; a strict > keeps the lowest index
// on ties.  ELU is monotone, so it is applied to the maximum.  Positions that no pool cell reads are never computed.
// The input is addressed through five strides (image, channel, depth, row, column), so the first layer reads the matching images as the
// batched GEMM wrote them (one plane per level) and the second layer reads the first one's channel-last output.  The pooled output is
// channel-last [image][cell][filter], or channel-first [image][filter][cell] (cf_out, the reference's flatten order for the last layer).
// Backward: the gradient of a pooled output reaches exactly one convolution position.  Weight and bias gradients are per-workgroup
// partial sums over a fixed share of the cells, added in workgroup order by a second launch; the input gradient is a gather (every input
// element visits the few cells whose footprint covers it, in a fixed order).  No float atomics: the bits are the same on every run.
#include "common.h"

namespace {

constexpr int C3_MAX_K = 4, C3_MAX_P = 4;
constexpr size_t C3_MAX_LDS = 160 * 1024;

struct c3_args {
  const float* x; long sxi, sxc, sxd, sxh, sxw;
  const float* wp; const float* bias; float* y; uint8_t* arg;
  const float* dy; float* dx; float* ws;
  int imgs, Cin, D, H, W, Cout, CoutPad, CinPad, St, PD, PH, PW, cf;
  int PHB, nchunk;      // forward only: pooled rows per workgroup, workgroups per (image, pooled depth)
  int nsplit;           // backward only: shares of an image's cells
};

static inline int pooled(int in, int K, int P, int St) {
  const int c = in - K + 1;
  return c < P ? 0 : (c - P) / St + 1;
}

__device__ __forceinline__ long out_index(const c3_args& a, long img, int cell, int f, int cells) {
  return a.cf ? (img * a.Cout + f) * cells + cell : (img * cells + cell) * a.Cout + f;
}

template <int K, int P>
__global__ __launch_bounds__(256) void conv3d_pool_fwd_kernel(const c3_args a) {
  extern __shared__ float smem[];
  constexpr int DD = P + K - 1, P3 = P * P * P, TAPS = K * K * K;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int chunk = b % a.nchunk; b /= a.nchunk;
  const int pd = b % a.PD;
  const long img = b / a.PD;
  const int ph0 = chunk * a.PHB;
  const int nph = min(a.PHB, a.PH - ph0);
  const int HH = (nph - 1) * a.St + DD, WW = (a.PW - 1) * a.St + DD;
  const int HHmax = (a.PHB - 1) * a.St + DD;
  const int FG = a.CoutPad >> 2;
  float* __restrict__ xs = smem;                                            // [Cin][DD][HH][WW]
  float* __restrict__ wl = xs + ((a.Cin * DD * HHmax * WW + 3) & ~3);       // [Cin][TAPS][CoutPad]
  float* __restrict__ cand = wl + a.Cin * TAPS * a.CoutPad;                 // [cells][P3][CoutPad]
  {
    const int nw4 = a.Cin * TAPS * FG;
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.wp);
    for (int i = tid; i < nw4; i += 256) reinterpret_cast<f32x4*>(wl)[i] = src[i];
  }
  {
    const float* __restrict__ xg = a.x + img * a.sxi + (long)(pd * a.St) * a.sxd + (long)(ph0 * a.St) * a.sxh;
    const int total = a.Cin * DD * HH * WW;
    if (a.sxc == 1) {
      for (int i = tid; i < total; i += 256) {
        const int ci = i % a.Cin; int r = i / a.Cin;
        const int ww = r % WW; r /= WW;
        const int hh = r % HH; const int dd = r / HH;
        xs[((ci * DD + dd) * HH + hh) * WW + ww] = xg[ci + dd * a.sxd + hh * a.sxh + ww * a.sxw];
      }
    } else {
      for (int i = tid; i < total; i += 256) {
        const int ww = i % WW; int r = i / WW;
        const int hh = r % HH; r /= HH;
        const int dd = r % DD; const int ci = r / DD;
        xs[i] = xg[ci * a.sxc + dd * a.sxd + hh * a.sxh + ww * a.sxw];
      }
    }
  }
  __syncthreads();
  const int ncell = nph * a.PW;
  const int items = ncell * P * P * FG;
  for (int it = tid; it < items; it += 256) {
    const int fg = it % FG; int r = it / FG;
    const int hoff = r % P; r /= P;
    const int doff = r % P; const int c = r / P;
    const int pw = c % a.PW, lph = c / a.PW;
    float acc[P][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f = fg * 4 + u;
      const float bv = f < a.Cout ? a.bias[f] : 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) acc[j][u] = bv;
    }
    for (int ci = 0; ci < a.Cin; ++ci) {
#pragma unroll
      for (int kd = 0; kd < K; ++kd) {
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
          const float* __restrict__ xr = xs + ((ci * DD + doff + kd) * HH + lph * a.St + hoff + kh) * WW + pw * a.St;
          const float* __restrict__ wr = wl + ((ci * K + kd) * K + kh) * K * a.CoutPad + fg * 4;
          float xv[DD];
#pragma unroll
          for (int q = 0; q < DD; ++q) xv[q] = xr[q];
#pragma unroll
          for (int kw = 0; kw < K; ++kw) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + kw * a.CoutPad);
#pragma unroll
            for (int j = 0; j < P; ++j) {
#pragma unroll
              for (int u = 0; u < 4; ++u) acc[j][u] = __builtin_fmaf(xv[j + kw], wv[u], acc[j][u]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      f32x4 v = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
      *reinterpret_cast<f32x4*>(cand + (c * P3 + (doff * P + hoff) * P + j) * a.CoutPad + fg * 4) = v;
    }
  }
  __syncthreads();
  const int cells = a.PD * a.PH * a.PW;
  for (int it = tid; it < ncell * a.Cout; it += 256) {
    const int f = it % a.Cout, c = it / a.Cout;
    const float* __restrict__ cp = cand + c * P3 * a.CoutPad + f;
    float m = cp[0];
    int am = 0;
#pragma unroll
    for (int q = 1; q < P3; ++q) {
      const float v = cp[q * a.CoutPad];
      if (v > m) { m = v; am = q; }
    }
    const int cell = (pd * a.PH + ph0 + c / a.PW) * a.PW + c % a.PW;
    const long o = out_index(a, img, cell, f, cells);
    a.y[o] = m > 0.f ? m : expm1f(m);
    a.arg[o] = (uint8_t)am;
  }
}

// gradient that reaches the convolution position of pooled output o: ELU' from the saved output (1 if y > 0, else y + 1)
__device__ __forceinline__ float pre_grad(const c3_args& a, long o) {
  const float yv = a.y[o];
  return a.dy[o] * (yv > 0.f ? 1.f : yv + 1.f);
}

// one workgroup per (image, share of its cells): ws[block][f][t], t < Cin K^3 the weight taps of filter f in the weight's own order, t = Cin K^3 the bias.
// The share is walked in tiles of `tile` cells: the tile's gradients and window positions are staged once in LDS ([cell][filter]), then every
// thread adds the tile, in cell order, to each of its (filter, tap) outputs -- one broadcast LDS read pair, one gathered input and one fmaf per term.
template <int K, int P>
__global__ __launch_bounds__(256) void conv3d_pool_dw_kernel(const c3_args a, int tile) {
  extern __shared__ float smem[];
  constexpr int TAPS = K * K * K;
  float* __restrict__ gs = smem;                                             // [tile][Cout]
  int* __restrict__ ps = reinterpret_cast<int*>(smem + tile * a.Cout);      // [tile][Cout]
  const int T = a.Cin * TAPS, T1 = T + 1;
  const int cells = a.PD * a.PH * a.PW;
  const int split = blockIdx.x % a.nsplit;
  const long img = blockIdx.x / a.nsplit;
  const int cps = (cells + a.nsplit - 1) / a.nsplit;
  const int c0 = split * cps, c1 = min(cells, c0 + cps);
  const float* __restrict__ xi = a.x + img * a.sxi;
  float* __restrict__ out = a.ws + (long)blockIdx.x * a.Cout * T1;
  if (c0 >= c1)
    for (int o = threadIdx.x; o < a.Cout * T1; o += 256) out[o] = 0.f;
  for (int cb = c0; cb < c1; cb += tile) {
    const int nc = min(tile, c1 - cb);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * a.Cout; i += 256) {
      const int cl = i / a.Cout, f = i - cl * a.Cout, c = cb + cl;
      const long oi = out_index(a, img, c, f, cells);
      const int am = a.arg[oi];
      const int pw = c % a.PW, ph = (c / a.PW) % a.PH, pd = c / (a.PW * a.PH);
      gs[i] = pre_grad(a, oi);
      ps[i] = (int)((long)(pd * a.St + am / (P * P)) * a.sxd + (long)(ph * a.St + (am / P) % P) * a.sxh + (long)(pw * a.St + am % P) * a.sxw);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < a.Cout * T1; o += 256) {
      const int f = o / T1, t = o - f * T1;
      float acc = cb == c0 ? 0.f : out[o];
      if (t < T) {
        const int ci = t / TAPS, kk = t - ci * TAPS;
        const float* __restrict__ xt = xi + (ci * a.sxc + (kk / (K * K)) * a.sxd + ((kk / K) % K) * a.sxh + (kk % K) * a.sxw);
        for (int cl = 0; cl < nc; ++cl) acc = __builtin_fmaf(gs[cl * a.Cout + f], xt[ps[cl * a.Cout + f]], acc);
      } else {
        for (int cl = 0; cl < nc; ++cl) acc += gs[cl * a.Cout + f];
      }
      out[o] = acc;
    }
  }
}

// dw[f][t] += the workgroups' partials in workgroup order; db[f] likewise
__global__ __launch_bounds__(256) void conv3d_pool_dw_reduce_kernel(const float* __restrict__ ws, int blocks, int Cout, int T, float* __restrict__ dw,
                                                                    float* __restrict__ db) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int T1 = T + 1;
  if (o >= Cout * T1) return;
  const float s = partial_rows_sum(ws, blocks, (long)Cout * T1, o);
  const int f = o / T1, t = o - f * T1;
  if (t < T) dw[f * T + t] += s;
  else db[f] += s;
}

// one thread per (image, depth, row, column, group of 4 channels) of the input: every element written once
template <int K, int P>
__global__ __launch_bounds__(256) void conv3d_pool_dx_kernel(const c3_args a, long total) {
  constexpr int TAPS = K * K * K, REACH = P + K - 2;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= total) return;
  const int CG = a.CinPad >> 2;
  int cg, w_, h_, d_;
  long img;
  if (a.sxc == 1) {
    cg = (int)(i % CG); long r = i / CG;
    w_ = (int)(r % a.W); r /= a.W;
    h_ = (int)(r % a.H); r /= a.H;
    d_ = (int)(r % a.D); img = r / a.D;
  } else {
    w_ = (int)(i % a.W); long r = i / a.W;
    h_ = (int)(r % a.H); r /= a.H;
    d_ = (int)(r % a.D); r /= a.D;
    cg = (int)(r % CG); img = r / CG;
  }
  const int cells = a.PD * a.PH * a.PW;
  const int dlo = d_ < REACH ? 0 : (d_ - REACH + a.St - 1) / a.St, dhi = min(a.PD - 1, d_ / a.St);
  const int hlo = h_ < REACH ? 0 : (h_ - REACH + a.St - 1) / a.St, hhi = min(a.PH - 1, h_ / a.St);
  const int wlo = w_ < REACH ? 0 : (w_ - REACH + a.St - 1) / a.St, whi = min(a.PW - 1, w_ / a.St);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int pd = dlo; pd <= dhi; ++pd)
    for (int ph = hlo; ph <= hhi; ++ph)
      for (int pw = wlo; pw <= whi; ++pw) {
        const int cell = (pd * a.PH + ph) * a.PW + pw;
        const int bd = d_ - pd * a.St, bh = h_ - ph * a.St, bw = w_ - pw * a.St;
        for (int f = 0; f < a.Cout; ++f) {
          const long oi = out_index(a, img, cell, f, cells);
          const int am = a.arg[oi];
          const int kd = bd - am / (P * P), kh = bh - (am / P) % P, kw = bw - am % P;
          if ((unsigned)kd >= (unsigned)K || (unsigned)kh >= (unsigned)K || (unsigned)kw >= (unsigned)K) continue;
          const float g = pre_grad(a, oi);
          const f32x4 wv = *reinterpret_cast<const f32x4*>(a.wp + ((long)(f * TAPS + (kd * K + kh) * K + kw) * a.CinPad + cg * 4));
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(g, wv[u], acc[u]);
        }
      }
  float* __restrict__ dst = a.dx + img * a.sxi + (long)d_ * a.sxd + (long)h_ * a.sxh + (long)w_ * a.sxw;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (cg * 4 + u < a.Cin) dst[(cg * 4 + u) * a.sxc] = acc[u];
}

struct c3_plan { int PD, PH, PW, PHB, nchunk; size_t lds; };

static bool c3_shape(int Cin, int D, int H, int W, int Cout, int K, int P, int St, c3_plan* pl) {
  if (K < 1 || K > C3_MAX_K || P < 1 || P > C3_MAX_P || St < P) return false;
  pl->PD = pooled(D, K, P, St); pl->PH = pooled(H, K, P, St); pl->PW = pooled(W, K, P, St);
  if (pl->PD <= 0 || pl->PH <= 0 || pl->PW <= 0) return false;
  const int DD = P + K - 1, CoutPad = (Cout + 3) & ~3, FG = CoutPad / 4, WW = (pl->PW - 1) * St + DD;
  auto lds = [&](int phb) {
    const size_t xs = ((size_t)Cin * DD * ((phb - 1) * St + DD) * WW + 3) & ~(size_t)3;
    return 4 * (xs + (size_t)Cin * K * K * K * CoutPad + (size_t)phb * pl->PW * P * P * P * CoutPad);
  };
  int phb = 1;
  while (phb < pl->PH && phb * pl->PW * P * P * FG < 256 && lds(phb + 1) <= 64 * 1024) ++phb;
  pl->PHB = phb;
  pl->nchunk = (pl->PH + phb - 1) / phb;
  pl->lds = lds(phb);
  return pl->lds <= C3_MAX_LDS;
}

// the forward launch of one (K, P) instantiation; a slab above 48 KB needs the kernel's dynamic-LDS ceiling raised, once per instantiation
template <int K, int P>
static int c3_fwd_launch(const c3_args& a, long blocks, size_t lds, hipStream_t stream) {
  static bool raised = false;
  if (lds > 48 * 1024 && !raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3d_pool_fwd_kernel<K, P>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)C3_MAX_LDS) != hipSuccess)
      return NNR_ERR_LAUNCH;
    raised = true;
  }
  hipLaunchKernelGGL((conv3d_pool_fwd_kernel<K, P>), dim3((unsigned)blocks), dim3(256), lds, stream, a);
  return NNR_OK;
}

#define C3_DISPATCH(KERNEL)                                                                                        \
  switch (K * 8 + P) {                                                                                             \
    case 1 * 8 + 1: C3_LAUNCH(KERNEL, 1, 1); break; case 1 * 8 + 2: C3_LAUNCH(KERNEL, 1, 2); break; \
    case 1 * 8 + 3: C3_LAUNCH(KERNEL, 1, 3); break; case 1 * 8 + 4: C3_LAUNCH(KERNEL, 1, 4); break; \
    case 2 * 8 + 1: C3_LAUNCH(KERNEL, 2, 1); break; case 2 * 8 + 2: C3_LAUNCH(KERNEL, 2, 2); break; \
    case 2 * 8 + 3: C3_LAUNCH(KERNEL, 2, 3); break; case 2 * 8 + 4: C3_LAUNCH(KERNEL, 2, 4); break; \
    case 3 * 8 + 1: C3_LAUNCH(KERNEL, 3, 1); break; case 3 * 8 + 2: C3_LAUNCH(KERNEL, 3, 2); break; \
    case 3 * 8 + 3: C3_LAUNCH(KERNEL, 3, 3); break; case 3 * 8 + 4: C3_LAUNCH(KERNEL, 3, 4); break; \
    case 4 * 8 + 1: C3_LAUNCH(KERNEL, 4, 1); break; case 4 * 8 + 2: C3_LAUNCH(KERNEL, 4, 2); break; \
    case 4 * 8 + 3: C3_LAUNCH(KERNEL, 4, 3); break; case 4 * 8 + 4: C3_LAUNCH(KERNEL, 4, 4); break; \
    default: return NNR_ERR_UNSUPPORTED;                                                                           \
  }

}  // namespace

extern "C" int nnr_conv3d_pool_dims(int Cin, int D, int H, int W, int Cout, int K, int P, int St, int* PD, int* PH, int* PW) {
  c3_plan pl;
  if (Cin <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return NNR_ERR_ARG;
  if (!c3_shape(Cin, D, H, W, Cout, K, P, St, &pl)) return NNR_ERR_UNSUPPORTED;
  if (PD) *PD = pl.PD;
  if (PH) *PH = pl.PH;
  if (PW) *PW = pl.PW;
  return NNR_OK;
}

extern "C" int nnr_conv3d_pool_fwd(const float* x, long sxi, long sxc, long sxd, long sxh, long sxw, const float* wp, const float* bias, int imgs,
                                   int Cin, int D, int H, int W, int Cout, int K, int P, int St, int cf_out, float* y, uint8_t* arg,
                                   hipStream_t stream) {
  if (!x || !wp || !bias || !y || !arg || imgs < 0 || Cin <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return NNR_ERR_ARG;
  c3_plan pl;
  if (!c3_shape(Cin, D, H, W, Cout, K, P, St, &pl) || !al16(wp)) return NNR_ERR_UNSUPPORTED;
  const long blocks = (long)imgs * pl.PD * pl.nchunk;
  if (blocks > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  if (imgs == 0) return NNR_OK;
  c3_args a = {};
  a.x = x; a.sxi = sxi; a.sxc = sxc; a.sxd = sxd; a.sxh = sxh; a.sxw = sxw; a.wp = wp; a.bias = bias; a.y = y; a.arg = arg;
  a.imgs = imgs; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.CoutPad = (Cout + 3) & ~3; a.CinPad = (Cin + 3) & ~3; a.St = St;
  a.PD = pl.PD; a.PH = pl.PH; a.PW = pl.PW; a.PHB = pl.PHB; a.nchunk = pl.nchunk; a.cf = cf_out ? 1 : 0;
#define C3_LAUNCH(KERNEL, KK, PP)                                    \
  do {                                                               \
    const int rc_ = c3_fwd_launch<KK, PP>(a, blocks, pl.lds, stream); \
    if (rc_ != NNR_OK) return rc_;                                   \
  } while (0)
  C3_DISPATCH(conv3d_pool_fwd_kernel)
#undef C3_LAUNCH
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

static int c3_nsplit(int imgs, int cells) {
  int s = (512 + imgs - 1) / imgs;
  if (s > cells) s = cells;
  return s < 1 ? 1 : s;
}

extern "C" size_t nnr_conv3d_pool_bwd_ws_floats(int imgs, int Cin, int D, int H, int W, int Cout, int K, int P, int St) {
  c3_plan pl;
  if (imgs <= 0 || Cin <= 0 || Cout <= 0 || !c3_shape(Cin, D, H, W, Cout, K, P, St, &pl)) return 0;
  return (size_t)imgs * c3_nsplit(imgs, pl.PD * pl.PH * pl.PW) * Cout * ((size_t)Cin * K * K * K + 1);
}

extern "C" int nnr_conv3d_pool_bwd(const float* dy, const float* y, const uint8_t* arg, const float* x, long sxi, long sxc, long sxd, long sxh,
                                   long sxw, const float* wq, int imgs, int Cin, int D, int H, int W, int Cout, int K, int P, int St, int cf_out,
                                   float* dx, float* dw_accum, float* db_accum, float* ws, hipStream_t stream) {
  if (!dy || !y || !arg || !x || !wq || !dw_accum || !db_accum || !ws || imgs < 0 || Cin <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0)
    return NNR_ERR_ARG;
  c3_plan pl;
  if (!c3_shape(Cin, D, H, W, Cout, K, P, St, &pl) || !al16(wq)) return NNR_ERR_UNSUPPORTED;
  if (imgs == 0) return NNR_OK;
  c3_args a = {};
  a.x = x; a.sxi = sxi; a.sxc = sxc; a.sxd = sxd; a.sxh = sxh; a.sxw = sxw; a.wp = wq; a.y = const_cast<float*>(y); a.arg = const_cast<uint8_t*>(arg);
  a.dy = dy; a.dx = dx; a.ws = ws;
  a.imgs = imgs; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.CoutPad = (Cout + 3) & ~3; a.CinPad = (Cin + 3) & ~3; a.St = St;
  a.PD = pl.PD; a.PH = pl.PH; a.PW = pl.PW; a.cf = cf_out ? 1 : 0;
  a.nsplit = c3_nsplit(imgs, pl.PD * pl.PH * pl.PW);
  const int T = Cin * K * K * K;
  const long wblocks = (long)imgs * a.nsplit;
  const long total = (long)imgs * D * H * W * (a.CinPad >> 2);
  const long xblocks = (total + 255) / 256;
  if (wblocks > 0x7fffffffL || xblocks > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  if ((D - 1) * sxd + (H - 1) * sxh + (W - 1) * sxw > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;     // a window position inside an image is an int
  int tile = 4096 / Cout;
  tile = tile > 128 ? 128 : (tile < 1 ? 1 : tile);
  if ((size_t)tile * Cout * 8 > 48 * 1024) return NNR_ERR_UNSUPPORTED;
#define C3_LAUNCH(KERNEL, KK, PP) hipLaunchKernelGGL((KERNEL<KK, PP>), dim3((unsigned)wblocks), dim3(256), (size_t)tile * Cout * 8, stream, a, tile)
  C3_DISPATCH(conv3d_pool_dw_kernel)
#undef C3_LAUNCH
  NNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(conv3d_pool_dw_reduce_kernel, dim3((unsigned)((Cout * (T + 1) + 255) / 256)), dim3(256), 0, stream, (const float*)ws, (int)wblocks,
                     Cout, T, dw_accum, db_accum);
  NNR_CHECK_LAUNCH();
  if (dx) {
#define C3_LAUNCH(KERNEL, KK, PP) hipLaunchKernelGGL((KERNEL<KK, PP>), dim3((unsigned)xblocks), dim3(256), 0, stream, a, total)
    C3_DISPATCH(conv3d_pool_dx_kernel)
#undef C3_LAUNCH
    NNR_CHECK_LAUNCH();
  }
  return NNR_OK;
}
