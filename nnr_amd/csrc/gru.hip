// GRU recurrence for the GRU user encoder (replaces nn.GRU on a PackedSequence, userEncoders.py:287-332, and its autograd
// backward) on gfx950.  Same one-CU design as the Bi-LSTM of lstm.hip: the input projection of ALL [B, T] history slots is one
// GEMM of the gemm.hip family (dead slots are computed and ignored); what remains is the strictly sequential part
//     r = s(x_r + W_hr h) ; z = s(x_z + W_hz h) ; n = tanh(x_n + r (W_hn h + b_hn)) ; h' = (1 - z) n + z h.
// One workgroup owns a tile of 16 users for ALL their steps: there is no communication between workgroups of any kind.  A user's
// length is the COUNT of ones in its mask row (pack_padded_sequence semantics); row b runs for t < len[b] and keeps h frozen from
// then on, which equals the reference's sort / pack / de-sort path and needs no planner and no host sync.  A tile loops to its own
// longest user (bounded by the host argument T).
//
// Per step: h_{t-1}[16, H] . W_hh^T[H, 3H] on v_mfma_f32_16x16x4_f32 (exact fp32), W_hh streamed from L2 in the pre-swizzled
// fragment layout of lstm.hip, h_{t-1} in LDS (XOR-swizzled).  Every unit has FOUR slots [r, z, n_x, n_h] (p-order:
// p = (unit/16)*64 + (unit%16)*4 + slot): a lane reads the projected (x_r, x_z, x_n, b_hn) of its (user, unit) as one float4, finds
// the three recurrent products in its own accumulators, and writes back (r, z, n, W_hn h + b_hn) -- what the backward pass needs.
// The reset gate multiplies the recurrent half of the candidate INCLUDING b_hn, so b_hn travels in slot 3 of the projection's
// bias vector (the W_ih rows of slot 3 are zero) instead of being folded into x_n.
//
// Backward: one launch walks t downwards, overwrites the saved activations with the pre-activation gradients
// (dr, dz, dn, dn r) -- zero at every dead slot -- and carries dh_{t-1} = dh_t z + [dr, dz, dn r] . W_hh in registers (second,
// untransposed fragment image; slot 2 multiplies zero rows).  Everything else (dX, dW_ih, dW_hh, the bias sums) is a product of
// the GEMM family or a fixed-order column sum over that buffer: no float atomics anywhere.
#include "common.h"

namespace {

__device__ __forceinline__ int swz16(int r16) { return (4 - (r16 >> 2)) & 3; }
// LDS offset (floats) of element (row r, column u) in a K-contiguous [16][ld] tile
__device__ __forceinline__ int lds_off(int r, int u, int ld) {
  return r * ld + (u & ~15) + 4 * (((u >> 2) & 3) ^ swz16(r)) + (u & 3);
}

struct GruArgs {
  float* gates;              // [B*T, NP]  fwd: in = x.W_ihp^T + b_p, out = (r, z, n, W_hn h + b_hn); bwd: out = d(pre-activations)
  const unsigned char* mask; // fwd: [B, T]
  const float* h0;           // fwd: [B, H] or null
  const float* wfrag;        // fwd: wf [UB][3][KG][64][4] ; bwd: wb [UB][NP/16][64][4]
  float* hout;               // fwd: [B*T, H]  h_t at every live slot
  float* hprev;              // fwd out / bwd in: [B*T, H]  h_{t-1} at every live slot
  float* hfinal;             // fwd: [B, H]
  int* len;                  // fwd out / bwd in: [B]
  const float* dhf;          // bwd: dL/dh_final [B, H]
  float* dh0;                // bwd: [B, H] or null
  int B, T, H;
};

// lengths of the tile's 16 users -> LDS (fwd: counted from the mask rows and published; bwd: read back), returns the tile's maximum
__device__ __forceinline__ int tile_lengths(const GruArgs& a, int s0, int* slen, bool count) {
  const int tid = threadIdx.x;
  if (tid < 16) {
    const int b = s0 + tid;
    int n = 0;
    if (b < a.B) {
      if (count) {
        const unsigned char* m = a.mask + (long)b * a.T;
        for (int t = 0; t < a.T; ++t) n += m[t] != 0;
        a.len[b] = n;
      } else {
        n = a.len[b];
      }
      n = min(max(n, 0), a.T);
    }
    slen[tid] = n;
  }
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) tmax = max(tmax, slen[i]);
  return tmax;
}

// ------------------------------------------------------------------------------------------------ forward
template <int UB>
__global__ __launch_bounds__((UB > 4 ? 16 : 4) * 64) void gru_fwd_kernel(GruArgs a) {
  constexpr int NW = UB > 4 ? 16 : 4, NT = NW * 64;      // one 16-unit block per wave
  constexpr int HP = UB * 16, NP = UB * 64, KG = UB;
  const int H = a.H, T = a.T;
  const int s0 = blockIdx.x * 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, kk = lane >> 4;
  __shared__ __attribute__((aligned(16))) float hbuf[2][16 * HP];
  __shared__ int slen[16];
  for (int i = tid; i < 2 * 16 * HP; i += NT) (&hbuf[0][0])[i] = 0.f;
  const int tmax = tile_lengths(a, s0, slen, true);        // (barrier inside: the zero fill above is complete)
  if (a.h0) {
    for (int i = tid; i < 16 * H; i += NT) {
      const int row = i / H, u = i - row * H;
      if (s0 + row < a.B) hbuf[0][lds_off(row, u, HP)] = a.h0[(long)(s0 + row) * H + u];
    }
    __syncthreads();
  }
  const bool own = w < UB;
  const int ub = own ? w : 0, unit = ub * 16 + r;
  int mylen[4];
  float h[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    mylen[e] = slen[kk * 4 + e];
    h[e] = hbuf[0][lds_off(kk * 4 + e, unit, HP)];
  }

  int cur = 0;
  // W_hh fragments are the same every step: the (kg + 1) % KG prefetch wraps around into the next step
  const f32x4* wf = reinterpret_cast<const f32x4*>(a.wfrag) + ((long)ub * 3 * KG) * 64 + lane;
  f32x4 bcur[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) bcur[g] = wf[(g * KG + 0) * 64];
  auto load_x = [&](int t, f32x4 (&x)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (own && t < mylen[e])
        x[e] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.gates + ((long)(s0 + kk * 4 + e) * T + t) * NP + ub * 64 + r * 4));
    }
  };
  f32x4 x[4];
  load_x(0, x);
  for (int t = 0; t < tmax; ++t) {
    const float* hc = hbuf[cur];
    float* hn = hbuf[cur ^ 1];
    if (own) {
      f32x4 acc[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 bnxt[3];
      // not unrolled: hipcc otherwise hoists the fragment loads of several k-groups and spills (62 dwords per lane at H = 200)
#pragma unroll 1
      for (int kg = 0; kg < KG; ++kg) {
        const int kn = (kg + 1 < KG) ? kg + 1 : 0;
#pragma unroll
        for (int g = 0; g < 3; ++g) bnxt[g] = wf[(g * KG + kn) * 64];
        __builtin_amdgcn_sched_barrier(0);      // keep the prefetch ahead of the MFMAs (see lstm.hip)
        const f32x4 af = *reinterpret_cast<const f32x4*>(&hc[r * HP + kg * 16 + 4 * (kk ^ swz16(r))]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int g = 0; g < 3; ++g)
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bcur[g][i], acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) bcur[g] = bnxt[g];
      }
      // lane-local cell update: the lane holds (row = kk*4 + e, unit = ub*16 + r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = kk * 4 + e;
        if (t < mylen[e]) {
          const long grow = (long)(s0 + row) * T + t;
          const float gr = fast_sigmoid(acc[0][e] + x[e][0]);
          const float gz = fast_sigmoid(acc[1][e] + x[e][1]);
          const float hh = acc[2][e] + x[e][3];
          const float gn = fast_tanh(x[e][2] + gr * hh);
          const float hv = (1.f - gz) * gn + gz * h[e];
          *reinterpret_cast<f32x4*>(a.gates + grow * NP + ub * 64 + r * 4) = f32x4{gr, gz, gn, hh};
          if (unit < H) {
            a.hprev[grow * H + unit] = h[e];
            a.hout[grow * H + unit] = hv;
          }
          h[e] = hv;
        }
        hn[lds_off(row, unit, HP)] = h[e];        // a user past its length keeps h
      }
    }
    if (t + 1 < tmax) load_x(t + 1, x);           // in flight across the barrier and the next step's MFMA loop
    __syncthreads();
    cur ^= 1;
  }
  if (own && unit < H) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = s0 + kk * 4 + e;
      if (b < a.B) a.hfinal[(long)b * H + unit] = h[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// Per step: (1) lane-local pre-activation gradients from the saved activations -> tile in LDS (+ global, in place over the
// saved activations);  (2) dh_{t-1} = dh_t z + tile[16, NP] . W_hh on the matrix cores; dh stays in the lane that needs it next.
template <int UB>
__global__ __launch_bounds__((UB > 4 ? 16 : 4) * 64) void gru_bwd_kernel(GruArgs a) {
  constexpr int NW = UB > 4 ? 16 : 4, NT = NW * 64;
  constexpr int NP = UB * 64, KGB = NP / 16;
  constexpr int DLD = NP + 16;             // row stride = 4 (mod 16) 16-byte chunks: the swizzle needs it
  const int H = a.H, T = a.T;
  const int s0 = blockIdx.x * 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, kk = lane >> 4;
  __shared__ __attribute__((aligned(16))) float dg[16 * DLD];
  __shared__ int slen[16];
  const int tmax = tile_lengths(a, s0, slen, false);
  // dead slots (t >= len[b]) hold the projection of padding: their gradient is zero
  {
    constexpr int C4 = NP / 4;
    const int total = 16 * T * C4;
    for (int i = tid; i < total; i += NT) {
      const int c = i % C4, q = i / C4, t = q % T, row = q / T;
      if (s0 + row < a.B && t >= slen[row])
        *reinterpret_cast<f32x4*>(a.gates + ((long)(s0 + row) * T + t) * NP + c * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  const bool own = w < UB;
  const int ub = own ? w : 0, unit = ub * 16 + r;
  int mylen[4];
  float dhr[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = s0 + kk * 4 + e;
    mylen[e] = slen[kk * 4 + e];
    dhr[e] = (own && b < a.B && unit < H) ? a.dhf[(long)b * H + unit] : 0.f;
  }
  // software-pipelined inputs of the gradient phase (loaded one step ahead, under the MFMA phase)
  f32x4 in_g[4];
  float in_hp[4];
  auto load_inputs = [&](int t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      in_g[e] = f32x4{0.f, 0.f, 0.f, 0.f};
      in_hp[e] = 0.f;
      if (own && t < mylen[e]) {
        const long grow = (long)(s0 + kk * 4 + e) * T + t;
        in_g[e] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.gates + grow * NP + ub * 64 + r * 4));
        if (unit < H) in_hp[e] = __builtin_nontemporal_load(a.hprev + grow * H + unit);
      }
    }
  };
  if (tmax > 0) load_inputs(tmax - 1);
  constexpr int PF = 4;
  static_assert(KGB % PF == 0, "prefetch ring must divide the fragment count");
  const f32x4* wb = reinterpret_cast<const f32x4*>(a.wfrag) + (long)ub * KGB * 64 + lane;
  f32x4 ring[PF];
#pragma unroll
  for (int j = 0; j < PF; ++j) ring[j] = wb[j * 64];

  for (int t = tmax - 1; t >= 0; --t) {
    float keep[4];
    // ---- (1) pre-activation gradients
    if (own) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = kk * 4 + e;
        f32x4 dgv = {0.f, 0.f, 0.f, 0.f};
        keep[e] = dhr[e];                         // a dead step passes dh through unchanged
        if (t < mylen[e]) {
          const float gr = in_g[e][0], gz = in_g[e][1], gn = in_g[e][2], hh = in_g[e][3];
          const float dh = dhr[e];
          const float dn = dh * (1.f - gz) * (1.f - gn * gn);
          dgv[0] = dn * hh * gr * (1.f - gr);
          dgv[1] = dh * (in_hp[e] - gn) * gz * (1.f - gz);
          dgv[2] = dn;
          dgv[3] = dn * gr;
          keep[e] = dh * gz;
          *reinterpret_cast<f32x4*>(a.gates + ((long)(s0 + row) * T + t) * NP + ub * 64 + r * 4) = dgv;
        }
        *reinterpret_cast<f32x4*>(&dg[lds_off(row, ub * 64 + r * 4, DLD)]) = dgv;
      }
    }
    __syncthreads();
    if (t > 0) load_inputs(t - 1);
    // ---- (2) dh_prev[16, HP] = tile[16, NP] . W_hh (p-order rows; slot 2 rows are zero)
    if (own) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int kg = 0; kg < KGB; ++kg) {
        const int kn = (kg + PF < KGB) ? kg + PF : kg + PF - KGB;     // wraps into the next step
        const f32x4 af = *reinterpret_cast<const f32x4*>(&dg[r * DLD + kg * 16 + 4 * (kk ^ swz16(r))]);
        const f32x4 b = ring[kg % PF];
        ring[kg % PF] = wb[kn * 64];
        __builtin_amdgcn_sched_barrier(0);      // pin the refill ahead of the MFMAs
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], b[i], acc, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) dhr[e] = acc[e] + keep[e];
    }
    __syncthreads();
  }
  if (a.dh0 && own && unit < H) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = s0 + kk * 4 + e;
      if (b < a.B) a.dh0[(long)b * H + unit] = dhr[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight (un)packing
__device__ __forceinline__ int slot_gate_x(int slot) { return slot < 3 ? slot : -1; }                       // W_ih rows: r, z, n, none
__device__ __forceinline__ int slot_gate_h(int slot) { return slot < 2 ? slot : (slot == 3 ? 2 : -1); }     // W_hh rows: r, z, none, n

__global__ void gru_pack_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                const float* __restrict__ b_hh, int H, int D, int UB, float* __restrict__ w_ihp,
                                float* __restrict__ b_p, float* __restrict__ wf, float* __restrict__ wb) {
  const int NP = UB * 64, KG = UB, KGB = NP / 16;
  const long n_ihp = (long)NP * D, n_b = NP, n_wf = (long)UB * 3 * KG * 256, n_wb = (long)UB * KGB * 256;
  const long total = n_ihp + n_b + n_wf + n_wb;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long i = idx;
    if (i < n_ihp) {                       // w_ihp[p][d]
      const int d = i % D, p = i / D;
      const int unit = (p / 64) * 16 + (p % 64) / 4, g = slot_gate_x(p % 4);
      w_ihp[i] = (unit < H && g >= 0) ? w_ih[(long)(g * H + unit) * D + d] : 0.f;
      continue;
    }
    i -= n_ihp;
    if (i < n_b) {                         // b_p[p]: (b_ir + b_hr, b_iz + b_hz, b_in, b_hn)
      const int p = i, unit = (p / 64) * 16 + (p % 64) / 4, s = p % 4;
      float v = 0.f;
      if (unit < H) v = s < 2 ? b_ih[s * H + unit] + b_hh[s * H + unit] : (s == 2 ? b_ih[2 * H + unit] : b_hh[2 * H + unit]);
      b_p[i] = v;
      continue;
    }
    i -= n_b;
    if (i < n_wf) {                        // wf[ub][g][kg][lane][ii] = w_hh[g*H + ub*16 + (lane&15)][16kg + 4(lane>>4) + ii]
      const int ii = i & 3, lane = (i >> 2) & 63; long q = i >> 8;
      const int kg = q % KG; q /= KG; const int g = q % 3; const int ub = q / 3;
      const int unit = ub * 16 + (lane & 15), k = 16 * kg + 4 * (lane >> 4) + ii;
      wf[i] = (unit < H && k < H) ? w_hh[(long)(g * H + unit) * H + k] : 0.f;
      continue;
    }
    i -= n_wf;
    {                                      // wb[ubn][kg][lane][ii] = w_hh[row(p)][ubn*16 + (lane&15)],  p = 16kg + 4(lane>>4) + ii
      const int ii = i & 3, lane = (i >> 2) & 63; long q = i >> 8;
      const int kg = q % KGB; const int ubn = q / KGB;
      const int p = 16 * kg + 4 * (lane >> 4) + ii;
      const int unit = (p / 64) * 16 + (p % 64) / 4, g = slot_gate_h(p % 4), col = ubn * 16 + (lane & 15);
      wb[i] = (unit < H && col < H && g >= 0) ? w_hh[(long)(g * H + unit) * H + col] : 0.f;
    }
  }
}

// dw_ihp [NP, D], db_p [NP], dw_hhp [NP, H]  ->  += into the gradients in nn.GRU's parameter layout (one writer per element)
__global__ void gru_unpack_kernel(const float* __restrict__ dw_ihp, const float* __restrict__ db_p, const float* __restrict__ dw_hhp,
                                  int H, int D, float* __restrict__ dw_ih, float* __restrict__ dw_hh, float* __restrict__ db_ih,
                                  float* __restrict__ db_hh) {
  const long n_ih = (long)3 * H * D, n_hh = (long)3 * H * H, n_b = 3 * H;
  const long total = n_ih + n_hh + n_b;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long i = idx;
    if (i < n_ih) {
      const int d = i % D, row = i / D, g = row / H, unit = row % H;
      dw_ih[i] += dw_ihp[(long)((unit / 16) * 64 + (unit % 16) * 4 + g) * D + d];
      continue;
    }
    i -= n_ih;
    if (i < n_hh) {
      const int k = i % H, row = i / H, g = row / H, unit = row % H;
      dw_hh[i] += dw_hhp[(long)((unit / 16) * 64 + (unit % 16) * 4 + (g == 2 ? 3 : g)) * H + k];
      continue;
    }
    i -= n_hh;
    {
      const int row = i, g = row / H, unit = row % H, p0 = (unit / 16) * 64 + (unit % 16) * 4;
      db_ih[row] += db_p[p0 + g];
      db_hh[row] += db_p[p0 + (g == 2 ? 3 : g)];
    }
  }
}

// y[b, :] = 0 for users without history (the reference's zero rows: not tanh(dec.bias))
__global__ void gru_zero_empty_kernel(float* __restrict__ y, const int* __restrict__ len, int B, int D) {
  const long n = (long)B * D;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    if (len[i / D] <= 0) y[i] = 0.f;
}
// dz = dy (1 - y^2) for y = tanh(z), zero for users without history
__global__ void gru_tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const int* __restrict__ len, int B, int D,
                                    float* __restrict__ dz) {
  const long n = (long)B * D;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = y[i];
    dz[i] = len[i / D] > 0 ? dy[i] * (1.f - v * v) : 0.f;
  }
}

template <int UB>
int launch_gru(const GruArgs& a, bool backward, hipStream_t s) {
  dim3 grid((a.B + 15) / 16), block((UB > 4 ? 16 : 4) * 64);
  if (backward) hipLaunchKernelGGL((gru_bwd_kernel<UB>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((gru_fwd_kernel<UB>), grid, block, 0, s, a);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

int gru_run(const GruArgs& a, bool backward, hipStream_t s) {
  int UB;
  if (a.B < 1) return NNR_ERR_ARG;
  if (nnr_gru_dims(a.H, a.T, &UB, nullptr, nullptr) != NNR_OK) return NNR_ERR_UNSUPPORTED;
  switch (UB) {
    case 1: return launch_gru<1>(a, backward, s);
    case 2: return launch_gru<2>(a, backward, s);
    case 3: return launch_gru<3>(a, backward, s);
    case 4: return launch_gru<4>(a, backward, s);
    case 5: return launch_gru<5>(a, backward, s);
    case 6: return launch_gru<6>(a, backward, s);
    case 7: return launch_gru<7>(a, backward, s);
    case 8: return launch_gru<8>(a, backward, s);
    case 9: return launch_gru<9>(a, backward, s);
    case 10: return launch_gru<10>(a, backward, s);
    case 11: return launch_gru<11>(a, backward, s);
    case 12: return launch_gru<12>(a, backward, s);
    case 13: return launch_gru<13>(a, backward, s);
    case 14: return launch_gru<14>(a, backward, s);
    case 15: return launch_gru<15>(a, backward, s);
    case 16: return launch_gru<16>(a, backward, s);
  }
  return NNR_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int nnr_gru_dims(int H, int T, int* UB, int* HP, int* NP) {
  const int ub = (H + 15) / 16;
  if (UB) *UB = ub;
  if (HP) *HP = ub * 16;
  if (NP) *NP = ub * 64;
  return (H >= 1 && H <= 256 && T >= 1 && T <= 255) ? NNR_OK : NNR_ERR_UNSUPPORTED;
}

extern "C" int nnr_gru_pack_weights(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int H, int D,
                                    float* w_ihp, float* b_p, float* wf, float* wb, hipStream_t stream) {
  int UB;
  if (!w_ih || !w_hh || !b_ih || !b_hh || !w_ihp || !b_p || !wf || !wb || D < 1) return NNR_ERR_ARG;
  if (nnr_gru_dims(H, 1, &UB, nullptr, nullptr) != NNR_OK) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gru_pack_kernel, dim3(512), dim3(256), 0, stream, w_ih, w_hh, b_ih, b_hh, H, D, UB, w_ihp, b_p, wf, wb);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_gru_unpack_grads(const float* dw_ihp, const float* db_p, const float* dw_hhp, int H, int D, float* dw_ih,
                                    float* dw_hh, float* db_ih, float* db_hh, hipStream_t stream) {
  if (!dw_ihp || !db_p || !dw_hhp || !dw_ih || !dw_hh || !db_ih || !db_hh || D < 1) return NNR_ERR_ARG;
  if (nnr_gru_dims(H, 1, nullptr, nullptr, nullptr) != NNR_OK) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gru_unpack_kernel, dim3(512), dim3(256), 0, stream, dw_ihp, db_p, dw_hhp, H, D, dw_ih, dw_hh, db_ih, db_hh);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_gru_fwd(float* gates, const unsigned char* mask, const float* h0, const float* wf, int B, int T, int H,
                           float* hout, float* hprev, float* hfinal, int* len, hipStream_t stream) {
  if (!gates || !mask || !wf || !hout || !hprev || !hfinal || !len) return NNR_ERR_ARG;
  GruArgs a = {};
  a.gates = gates; a.mask = mask; a.h0 = h0; a.wfrag = wf; a.hout = hout; a.hprev = hprev; a.hfinal = hfinal; a.len = len;
  a.B = B; a.T = T; a.H = H;
  return gru_run(a, false, stream);
}

extern "C" int nnr_gru_bwd(float* gates, const int* len, const float* hprev, const float* wb, const float* dhfinal, int B, int T,
                           int H, float* dh0, hipStream_t stream) {
  if (!gates || !len || !hprev || !wb || !dhfinal) return NNR_ERR_ARG;
  GruArgs a = {};
  a.gates = gates; a.len = const_cast<int*>(len); a.hprev = const_cast<float*>(hprev); a.wfrag = wb; a.dhf = dhfinal; a.dh0 = dh0;
  a.B = B; a.T = T; a.H = H;
  return gru_run(a, true, stream);
}

extern "C" int nnr_gru_zero_empty(float* y, const int* len, int B, int D, hipStream_t stream) {
  if (!y || !len || B < 1 || D < 1) return NNR_ERR_ARG;
  hipLaunchKernelGGL(gru_zero_empty_kernel, dim3(min(1024, (B * D + 255) / 256)), dim3(256), 0, stream, y, len, B, D);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_gru_tanh_bwd(const float* dy, const float* y, const int* len, int B, int D, float* dz, hipStream_t stream) {
  if (!dy || !y || !len || !dz || B < 1 || D < 1) return NNR_ERR_ARG;
  hipLaunchKernelGGL(gru_tanh_bwd_kernel, dim3(min(1024, (B * D + 255) / 256)), dim3(256), 0, stream, dy, y, len, B, D, dz);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
