// Top-K recommendation: idx / score [n_user, K] = the K eligible news rows of the largest inner products
// <user[u], reps[r]>, without the [n_user, n_reps] score matrix ever reaching global memory.
//
// topk_tile_kernel: one workgroup (4 waves) owns a tile of 64 users and a contiguous range of 128-news tiles, which it walks in ascending
// order.  Per news tile the 64 x 128 scores are accumulated on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32; wave w holds the 32 users
// (w & 1) x the 64 news (w >> 1) in two accumulators), with the D dimension streamed through LDS in slabs of 32 (k-major images; the
// next slab travels in registers under the current one's products; the tail of the last slab is zero-filled, which leaves every sum as it is).
// The finished tile goes to LDS (over the operand images), ineligible positions are overwritten with -inf -- columns beyond n_reps
// or with valid == 0 as whole columns, the exclusion lists scatter-wise, one store per (user, entry) that falls into the tile -- and each
// wave folds its 16 users' rows into their running lists: a list is 64 (score, row) entries in LDS, one per lane, sorted by score
// descending; a score is admitted only when it is strictly greater than the list's K-th entry and goes behind every entry >= it.
// News ascend, so an earlier (smaller) row wins every tie, inside the list and at the cut.  After the first tiles almost nothing passes
// the ballot: a user costs one broadcast read, two reads and two compares per tile.
// Launches with few user tiles split the news tiles over `splits` workgroups per user tile, which leave [n_user, splits, K] partial lists
// in the workspace; topk_merge_kernel (one wave per user) folds them in (split, k) order with the same admission rule, which is the
// order (score descending, row ascending) again.  A score is one fmaf chain over d ascending whatever the tile, the split or the load
// path, and the selection is a function of the scores and rows alone: nothing depends on the launch shape.  No atomics.
//
// Full-pool ranks (nnr_pool_ranks): the same walk (score_tile_walk, shared by both kernels) with another fold.
// pool_rank_target_kernel computes each named target's score as the literal fmaf chain, which is the tile's value to the bit, and its
// eligibility; pool_rank_tile_kernel counts per (user, target) the tile entries that precede the target -- greater, or equal with a
// smaller row: one compare of 64-bit (score, row) keys -- as the population counts of two ballots, and per user the entries that are not -inf.  A counter is touched by the one
// wave that owns its user: LDS for the first 2048 targets of a user tile, the counter's own destination in global memory beyond.  With
// splits the partial counts [n_target + n_user, splits] go through the workspace and pool_rank_merge_kernel adds them in split order.
#include <limits.h>
#include "common.h"

namespace {
constexpr int TK_TU = 64, TK_TN = 128, TK_KS = 32;         // user tile, news tile, slab of the D dimension
constexpr int TK_SA = TK_TU + 2, TK_SB = TK_TN + 2;        // k-major image strides: = 2 mod 8, so a slab's stores are at most 2-way on a bank
constexpr int TK_STAGE = TK_KS * (TK_SA + TK_SB);          // floats of one slab's two operand images (25 KB; the score tile needs 32 KB)
constexpr int TK_WORKGROUPS_WANTED = 2048;                 // workgroups a launch aims for: 4 rounds of 2 per CU on 256 CUs
constexpr int TK_MAX_SPLITS = 256;

__host__ __device__ inline int topk_splits(long n_user, long n_reps) {
  const long ut = (n_user + TK_TU - 1) / TK_TU, nt = (n_reps + TK_TN - 1) / TK_TN;
  long s = (TK_WORKGROUPS_WANTED + ut - 1) / ut;
  if (s > nt / 2) s = nt / 2;                               // a split walks at least two tiles: its first slab's latency is paid once
  if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

// The candidate (s, r) into a list sorted by score descending, one entry per lane: behind every entry >= s, the rest moves down one lane
// and the last entry falls off.  Wave-uniform s, r and control flow.
__device__ __forceinline__ void list_insert(float& ls, int& li, float s, int r, int lane) {
  const int p = __popcll(__ballot(ls >= s));               // the entries >= s are a prefix of the lanes: the list is sorted
  const float us = __shfl_up(ls, 1, 64);
  const int ui = __shfl_up(li, 1, 64);
  if (lane == p) { ls = s; li = r; }
  else if (lane > p) { ls = us; li = ui; }
}
// The candidates c (row cr; lanes of `m`) in ascending lane order, each admitted only if strictly greater than the K-th entry.
__device__ __forceinline__ void list_admit(float& ls, int& li, unsigned long long m, float c, int cr, int K, int lane) {
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const float s = __shfl(c, src, 64);
    const int r = __shfl(cr, src, 64);
    if (s > __shfl(ls, K - 1, 64)) list_insert(ls, li, s, r, lane);
  }
}

// ------------------------------------------------------------------------------------------------ the archive form
// A user row of the archive entry points is A vectors, lda floats apart; the plain entry points launch the ARCH = false instantiations, which
// never read this.
struct Archives { int A, lda; float scale; };

// combine of include/nnr_hip.h, one archive at a time: the state (m, den, num) after archives 0 .. a from the state after 0 .. a - 1 and
// s = s_a.  THE one statement of the sequence: the tile walk and the target pre-pass both call it, every operation is an explicitly rounded
// one and contraction is off, so the two sites cannot differ.  `first` (a == 0) is uniform over the launch.
__device__ __forceinline__ void archive_fold(bool first, float s, float scale, float& m, float& den, float& num) {
#pragma clang fp contract(off)
  if (first) { m = s; den = 1.f; num = s; return; }
  const bool up = scale < 0.f ? s < m : s > m;             // s is the new extreme: the state is rescaled to it; otherwise s joins the state
  const float e = expf(__fmul_rn(scale, up ? __fsub_rn(m, s) : __fsub_rn(s, m)));
  den = __fmaf_rn(up ? den : 1.f, e, up ? 1.f : den);
  num = __fmaf_rn(up ? num : s, e, up ? s : num);
  m = up ? s : m;
}
__device__ __forceinline__ float archive_score(float den, float num) { return __fdiv_rn(num, den); }

// The walk both kernels of this file share: the 64 users from u0 against the news tiles t_begin .. t_end - 1 in ascending order.  For each
// tile the finished, masked 64 x 128 scores stand in `tile` ([user][news]; -inf over every ineligible position) and fold(n0) is called by
// all 256 threads behind a barrier; the next tile's first barrier guards `tile` against its readers, so fold needs none of its own.
// ARCH: a tile is walked once per archive a = 0 .. A - 1 (the news slabs are read again, from L2), each pass leaves the chains s_a in the
// accumulators and archive_fold takes them into 96 registers of state per lane; the tile that reaches LDS holds the combined scores, and
// everything behind that point is the plain walk's.  The operand stream never stops: the last slab of a pass prefetches the next pass's first.
template <bool VEC, bool ARCH, class Fold>
__device__ __forceinline__ void score_tile_walk(float* tile, const float* __restrict__ user, long n_user, int ldu, const float* __restrict__ reps,
                                                long n_reps, int ldr, int D, const uint8_t* __restrict__ valid, const int* __restrict__ exclude,
                                                int E, int ld_ex, long u0, long t_begin, long t_end, const Archives& ar, Fold&& fold) {
  static_assert(TK_STAGE <= TK_TU * TK_TN, "the operand images live inside the score tile");
  float* As = tile;                                         // [k][TK_SA]: As[k * TK_SA + u]
  float* Bs = tile + TK_KS * TK_SA;                         // [k][TK_SB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nslab = (D + TK_KS - 1) / TK_KS;

  // one slab of both operands, global -> registers: 2048 user floats and 4096 news floats over 256 threads
  float pre[24];
  auto gload = [&](long n0, int k0, int a) {
    const float* __restrict__ ua = ARCH ? user + (long)a * ar.lda : user;
    if (VEC) {                                              // thread: float4 column kq of rows r, r + 32, ...   (D % 4 == 0)
      const int kq = tid & 7, r = tid >> 3, k = k0 + 4 * kq;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const bool is_u = i < 2;
        const long row = is_u ? u0 + r + 32 * i : n0 + r + 32 * (i - 2);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < D && row < (is_u ? n_user : n_reps))
          v = *reinterpret_cast<const float4*>(is_u ? ua + row * ldu + k : reps + row * ldr + k);
        pre[4 * i] = v.x; pre[4 * i + 1] = v.y; pre[4 * i + 2] = v.z; pre[4 * i + 3] = v.w;
      }
    } else {                                                // thread: column k of rows r, r + 8, ...
      const int kk = tid & 31, r = tid >> 5, k = k0 + kk;
#pragma unroll
      for (int i = 0; i < 24; ++i) {
        const bool is_u = i < 8;
        const long row = is_u ? u0 + r + 8 * i : n0 + r + 8 * (i - 8);
        float v = 0.f;
        if (k < D && row < (is_u ? n_user : n_reps)) v = is_u ? ua[row * ldu + k] : reps[row * ldr + k];
        pre[i] = v;
      }
    }
  };
  auto lstore = [&]() {
    if (VEC) {
      const int kq = tid & 7, r = tid >> 3;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (i < 2) As[(4 * kq + c) * TK_SA + r + 32 * i] = pre[4 * i + c];
          else Bs[(4 * kq + c) * TK_SB + r + 32 * (i - 2)] = pre[4 * i + c];
        }
    } else {
      const int kk = tid & 31, r = tid >> 5;
#pragma unroll
      for (int i = 0; i < 24; ++i) {
        if (i < 8) As[kk * TK_SA + r + 8 * i] = pre[i];
        else Bs[kk * TK_SB + r + 8 * (i - 8)] = pre[i];
      }
    }
  };

  const int wu = (wave & 1) * 32, wn = (wave >> 1) * 64;   // this wave's 32 users x 64 news of the tile
  const int half = lane >> 5, l31 = lane & 31;
  const int A = ARCH ? ar.A : 1;
  if (t_begin < t_end) gload(t_begin * TK_TN, 0, 0);
  for (long t = t_begin; t < t_end; ++t) {
    const long n0 = t * TK_TN;
    f32x16 acc0, acc1;
    [[maybe_unused]] float m0[16], m1[16], den0[16], den1[16], num0[16], num1[16];   // ARCH: the combine state of this lane's 32 tile elements
    for (int a = 0; a < A; ++a) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
      for (int sl = 0; sl < nslab; ++sl) {
        __syncthreads();                                    // the previous slab's products / the previous tile's fold have read `tile`
        lstore();
        __syncthreads();
        if (sl + 1 < nslab) gload(n0, (sl + 1) * TK_KS, a);
        else if (ARCH && a + 1 < A) gload(n0, 0, a + 1);
        else if (t + 1 < t_end) gload(n0 + TK_TN, 0, 0);
#pragma unroll
        for (int s = 0; s < TK_KS / 2; ++s) {               // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
          const int k = 2 * s + half;
          const float a_ = As[k * TK_SA + wu + l31];
          const float b0 = Bs[k * TK_SB + wn + l31], b1 = Bs[k * TK_SB + wn + 32 + l31];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_, b0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_, b1, acc1, 0, 0, 0);
        }
      }
      if constexpr (ARCH) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float s0 = acc0[i], s1 = acc1[i];
          archive_fold(a == 0, s0, ar.scale, m0[i], den0[i], num0[i]);
          archive_fold(a == 0, s1, ar.scale, m1[i], den1[i], num1[i]);
          __builtin_amdgcn_sched_barrier(0);                // two exponentials in flight, not 32: their temporaries would not fit beside the state
        }
      }
    }
    if constexpr (ARCH) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { acc0[i] = archive_score(den0[i], num0[i]); acc1[i] = archive_score(den1[i], num1[i]); }
    }
    __syncthreads();                                        // every wave is done with the operand images
#pragma unroll
    for (int i = 0; i < 16; ++i) {                          // C/D: column = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
      const int u = wu + (i & 3) + 8 * (i >> 2) + 4 * half;
      tile[u * TK_TN + wn + l31] = acc0[i];
      tile[u * TK_TN + wn + 32 + l31] = acc1[i];
    }
    __syncthreads();
    {                                                       // columns out of the pool: thread = column tid & 127 of users (tid >> 7) * 32 ..
      const int j = tid & 127;
      const long r = n0 + j;
      if (r >= n_reps || (valid && valid[r] == 0)) {
        const int ub = (tid >> 7) * 32;
        for (int u = ub; u < ub + 32; ++u) tile[u * TK_TN + j] = -INFINITY;
      }
    }
    for (long p = tid; p < (long)TK_TU * E; p += 256) {            // exclusion lists: one store per entry that falls into this tile
      const int u = (int)(p / E), e = (int)(p - (long)u * E);
      if (u0 + u < n_user) {
        const long r = exclude[(u0 + u) * ld_ex + e];
        if (r >= n0 && r < n0 + TK_TN && r < n_reps) tile[u * TK_TN + (int)(r - n0)] = -INFINITY;
      }
    }
    __syncthreads();
    fold(t, n0);
  }
}

template <bool VEC, bool ARCH>
__global__ __launch_bounds__(256, ARCH && VEC ? 2 : 0) void topk_tile_kernel(const float* __restrict__ user, long n_user, int ldu, const float* __restrict__ reps,
                                                        long n_reps, int ldr, int D, const uint8_t* __restrict__ valid,
                                                        const int* __restrict__ exclude, int E, int ld_ex, int K, long user_tiles,
                                                        int splits, int* __restrict__ out_idx, float* __restrict__ out_score, Archives ar) {
  __shared__ float tile[TK_TU * TK_TN];                     // the score tile [user][news]; before that, the slab's operand images
  __shared__ float lst_s[TK_TU * 64];
  __shared__ int lst_i[TK_TU * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long ut = blockIdx.x % user_tiles;
  const int split = (int)(blockIdx.x / user_tiles);
  const long u0 = ut * TK_TU;
  const long nt = (n_reps + TK_TN - 1) / TK_TN;
  const long t_begin = nt * split / splits, t_end = nt * (split + 1) / splits;

  for (int u = wave * 16; u < wave * 16 + 16; ++u) {        // a wave's lists are its own from here to the end: no barrier guards them
    lst_s[u * 64 + lane] = -INFINITY;
    lst_i[u * 64 + lane] = -1;
  }
  score_tile_walk<VEC, ARCH>(tile, user, n_user, ldu, reps, n_reps, ldr, D, valid, exclude, E, ld_ex, u0, t_begin, t_end, ar, [&](long, long n0) {
    for (int u = wave * 16; u < wave * 16 + 16; ++u) {      // wave-uniform
      if (u0 + u >= n_user) break;
      const float thr = lst_s[u * 64 + K - 1];
      const float c0 = tile[u * TK_TN + lane], c1 = tile[u * TK_TN + 64 + lane];
      const unsigned long long m0 = __ballot(c0 > thr), m1 = __ballot(c1 > thr);
      if (m0 | m1) {
        float ls = lst_s[u * 64 + lane];
        int li = lst_i[u * 64 + lane];
        list_admit(ls, li, m0, c0, (int)(n0 + lane), K, lane);
        list_admit(ls, li, m1, c1, (int)(n0 + 64 + lane), K, lane);
        lst_s[u * 64 + lane] = ls;
        lst_i[u * 64 + lane] = li;
      }
    }
  });
  if (lane < K)
    for (int u = wave * 16; u < wave * 16 + 16; ++u) {
      if (u0 + u >= n_user) break;
      const long o = ((u0 + u) * splits + split) * K + lane;
      out_score[o] = lst_s[u * 64 + lane];
      out_idx[o] = lst_i[u * 64 + lane];
    }
}

// idx / score [n_user, K] from the partial lists [n_user, splits, K]: one wave per user, the entries in (split, k) order
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ ws_score, const int* __restrict__ ws_idx, long n_user,
                                                         int splits, int K, int* __restrict__ idx, float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_user) return;                                  // wave-uniform
  const int n = splits * K;
  const float* __restrict__ ps = ws_score + u * n;
  const int* __restrict__ pi = ws_idx + u * n;
  float ls = -INFINITY;
  int li = -1;
  for (int base = 0; base < n; base += 64) {
    const int e = base + lane;
    const float c = e < n ? ps[e] : -INFINITY;
    const int cr = e < n ? pi[e] : -1;
    const unsigned long long m = __ballot(c > __shfl(ls, K - 1, 64));
    list_admit(ls, li, m, c, cr, K, lane);
  }
  if (lane < K) {
    score[u * K + lane] = ls;
    idx[u * K + lane] = li;
  }
}

// ------------------------------------------------------------------------------------------------ full-pool ranks
// ahead[j] = the number of eligible rows that nnr_topk_scores would place before target j of its user, for targets (t_off, t_news) that
// the caller names: the same walk, with counters where the top-K kernel keeps lists.
constexpr int PR_CAP = 2048;                               // targets of one 64-user tile whose key and counter live in LDS: 24 KB

// (score, row) as one unsigned number whose order is "score ascending, equal scores by DESCENDING row": the float's bits made monotone (-0
// first turned into +0, so that scores which compare equal have equal keys) above the complement of the row.  An entry precedes a target
// exactly when its key is greater.  Finite scores and -inf; rows from 0.
__device__ __forceinline__ unsigned long long rank_key(float s, int r) {
  const unsigned b = __float_as_uint(s + 0.f);
  const unsigned o = b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
  return ((unsigned long long)o << 32) | (unsigned)~r;
}

// t_score[j] = the header's chain for (user of j, t_news[j]); ahead[j] = 0 for an eligible target and -1 for an ineligible one (the
// counters behind it leave a -1 alone).  One thread per target; its user is the last u with t_off[u] <= j.  ARCH: one chain per archive,
// combined by archive_fold as the tile walk combines them.
template <bool ARCH>
__global__ __launch_bounds__(256) void pool_rank_target_kernel(const float* __restrict__ user, long n_user, int ldu, const float* __restrict__ reps,
                                                               long n_reps, int ldr, int D, const uint8_t* __restrict__ valid,
                                                               const int* __restrict__ exclude, int E, int ld_ex, const int* __restrict__ t_off,
                                                               const int* __restrict__ t_news, long n_target, int* __restrict__ ahead,
                                                               float* __restrict__ t_score, Archives ar) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_target) return;
  long lo = 0, hi = n_user;                                 // t_off[lo] <= j < t_off[hi] (t_off[0] = 0, t_off[n_user] = n_target)
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (t_off[mid] <= j) lo = mid; else hi = mid;
  }
  const long u = lo, r = t_news[j];
  if (r < 0 || r >= n_reps) {                               // not a row of the table: nothing is read for it
    t_score[j] = __builtin_nanf("");
    ahead[j] = -1;
    return;
  }
  const float* __restrict__ b = reps + r * ldr;
  float acc = 0.f;
  [[maybe_unused]] float m = 0.f, den = 1.f, num = 0.f;
  for (int k = 0; k < (ARCH ? ar.A : 1); ++k) {
    const float* __restrict__ a = user + u * ldu + (ARCH ? (long)k * ar.lda : 0);
    acc = 0.f;
    for (int d = 0; d < D; ++d) acc = __fmaf_rn(a[d], b[d], acc);
    if (D % TK_KS) acc = __fmaf_rn(0.f, 0.f, acc);          // the tile's zero-filled tail, literally (it turns a -0 into +0 and nothing else)
    if constexpr (ARCH) archive_fold(k == 0, acc, ar.scale, m, den, num);
  }
  if constexpr (ARCH) acc = archive_score(den, num);
  bool el = !valid || valid[r] != 0;
  for (int e = 0; e < E; ++e) el = el && exclude[u * ld_ex + e] != (int)r;
  t_score[j] = acc;
  ahead[j] = el ? 0 : -1;
}

// cnt_t[j * splits + split] = the entries of this workgroup's news tiles that precede target j; cnt_u[u * splits + split] = the eligible
// ones among them.  A tile's targets are the contiguous range t_off[u0] .. t_off[u0 + 64); position p in it has its key and its counter
// in LDS while p < PR_CAP and works on global memory beyond that: the counter's own destination, read and written by ONE lane of the wave
// that owns the user, tile after tile.  Without splits the destination of a counter is ahead[j] itself, where the pre-pass left 0 or -1.
template <bool VEC, bool ARCH>
__global__ __launch_bounds__(256, ARCH && VEC ? 2 : 0) void pool_rank_tile_kernel(const float* __restrict__ user, long n_user, int ldu, const float* __restrict__ reps,
                                                             long n_reps, int ldr, int D, const uint8_t* __restrict__ valid,
                                                             const int* __restrict__ exclude, int E, int ld_ex, long user_tiles, int splits,
                                                             const int* __restrict__ t_off, const int* __restrict__ t_news,
                                                             const float* __restrict__ t_score, long n_target, int* cnt_t,
                                                             int* __restrict__ cnt_u, Archives ar) {
  __shared__ float tile[TK_TU * TK_TN];
  __shared__ unsigned long long tg_k[PR_CAP];              // rank_key of the tile's first PR_CAP targets
  __shared__ int tg_c[PR_CAP];                              // and their counters
  __shared__ int u_off[TK_TU + 1];                          // the targets of tile user u: u_off[u] .. u_off[u + 1] - 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long ut = blockIdx.x % user_tiles;
  const int split = (int)(blockIdx.x / user_tiles);
  const long u0 = ut * TK_TU;
  const long nt = (n_reps + TK_TN - 1) / TK_TN;
  const long t_begin = nt * split / splits, t_end = nt * (split + 1) / splits;   // never empty: topk_splits gives a split two tiles or more

  if (tid <= TK_TU) {                                       // clamped into 0 .. n_target: whatever t_off holds, no access leaves t_news / t_score
    const long u = u0 + tid < n_user ? u0 + tid : n_user;
    const long o = t_off[u];
    u_off[tid] = (int)(o < 0 ? 0 : (o > n_target ? n_target : o));
  }
  __syncthreads();
  const int tb = __builtin_amdgcn_readfirstlane(u_off[0]);  // (what LDS returns is the same in every lane; said so, the loops below stay scalar)
  {
    const int n = min(max(u_off[TK_TU] - tb, 0), PR_CAP);
    for (int p = tid; p < n; p += 256) {
      tg_k[p] = rank_key(t_score[tb + p], t_news[tb + p]);
      tg_c[p] = 0;
    }
  }
  __syncthreads();
  int psz = 0;                                              // lane l of a wave: the eligible entries of its user wave * 16 + l (l < 16)
  score_tile_walk<VEC, ARCH>(tile, user, n_user, ldu, reps, n_reps, ldr, D, valid, exclude, E, ld_ex, u0, t_begin, t_end, ar, [&](long t, long n0) {
    for (int u = wave * 16; u < wave * 16 + 16; ++u) {      // wave-uniform
      if (u0 + u >= n_user) break;
      const float c0 = tile[u * TK_TN + lane], c1 = tile[u * TK_TN + 64 + lane];
      const unsigned long long k0 = rank_key(c0, (int)(n0 + lane)), k1 = rank_key(c1, (int)(n0 + 64 + lane));
      const int np = __popcll(__ballot(c0 != -INFINITY)) + __popcll(__ballot(c1 != -INFINITY));
      if (lane == u - wave * 16) psz += np;
      const int b = max(__builtin_amdgcn_readfirstlane(u_off[u]) - tb, 0), e = __builtin_amdgcn_readfirstlane(u_off[u + 1]) - tb;
      for (int base = b; base < e; base += 64) {            // 64 targets at a time, one per lane
        const int p = base + lane;
        const bool live = p < e, in_lds = p < PR_CAP;
        unsigned long long kt = 0;
        if (live) kt = in_lds ? tg_k[p] : rank_key(t_score[tb + p], t_news[tb + p]);
        const int hi = (int)(kt >> 32), lo = (int)kt;
        int cnt = 0;
        const int m = min(64, e - base);
        for (int k = 0; k < m; ++k) {                       // target k of the 64, broadcast from its lane; scalar from here to the count
          const unsigned long long key = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, k) << 32) |
                                         (unsigned)__builtin_amdgcn_readlane(lo, k);
          const int c = __popcll(__builtin_amdgcn_ballot_w64(k0 > key)) + __popcll(__builtin_amdgcn_ballot_w64(k1 > key));
          if (lane == k) cnt = c;
        }
        if (live) {
          if (in_lds) tg_c[p] += cnt;
          else {
            int* q = cnt_t + (long)(tb + p) * splits + split;
            const int a = (splits > 1 && t == t_begin) ? 0 : *q;
            if (a >= 0) *q = a + cnt;
          }
        }
      }
    }
  });
  if (lane < 16 && u0 + wave * 16 + lane < n_user) cnt_u[(u0 + wave * 16 + lane) * splits + split] = psz;
  {                                                         // a wave's own counters: no barrier
    const int b = max(__builtin_amdgcn_readfirstlane(u_off[wave * 16]) - tb, 0), e = min(__builtin_amdgcn_readfirstlane(u_off[wave * 16 + 16]) - tb, PR_CAP);
    for (int p = b + lane; p < e; p += 64) {
      int* q = cnt_t + (long)(tb + p) * splits + split;
      if (splits > 1 || *q >= 0) *q = tg_c[p];
    }
  }
}

// ahead[j] = sum of ws[j, 0 .. splits) unless the pre-pass left -1 there; pool_size[u] = sum of ws[n_target + u, 0 .. splits); split order
__global__ __launch_bounds__(256) void pool_rank_merge_kernel(const int* __restrict__ ws, long n_target, long n_user, int splits,
                                                              int* __restrict__ ahead, int* __restrict__ pool_size) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_target + n_user) return;
  int sum = 0;
  for (int s = 0; s < splits; ++s) sum += ws[i * splits + s];
  if (i >= n_target) pool_size[i - n_target] = sum;
  else if (ahead[i] >= 0) ahead[i] = sum;
}
}  // namespace


extern "C" size_t nnr_pool_rank_workspace_bytes(long n_user, long n_reps, long n_target) {
  if (n_user < 1 || n_reps < 1 || n_target < 0 || n_user >= INT_MAX || n_reps > INT_MAX || n_target > INT_MAX) return 0;
  const int splits = topk_splits(n_user, n_reps);
  return splits > 1 ? (size_t)(n_target + n_user) * splits * sizeof(int) : 0;
}

extern "C" size_t nnr_topk_workspace_bytes(long n_user, long n_reps, int K) {
  if (n_user < 1 || n_reps < 1 || K < 1 || K > 64) return 0;
  const int splits = topk_splits(n_user, n_reps);
  return splits > 1 ? (size_t)n_user * splits * K * (sizeof(float) + sizeof(int)) : 0;
}

namespace {
// What the archive entry points check beyond their plain counterparts (A > 16 is refused behind the plain argument checks)
bool archives_ok(int ldu, int A, int lda, float scale, int D) {
  return A >= 1 && D >= 1 && lda >= D && (long)ldu >= (long)(A - 1) * lda + D && scale - scale == 0.f;
}

// The body of nnr_pool_ranks (ARCH = false: `ar` is not read by any kernel) and of nnr_pool_archive_ranks
template <bool ARCH>
int pool_ranks_run(const float* user, long n_user, int ldu, const Archives& ar, const float* reps, long n_reps, int ldr, int D,
                   const uint8_t* valid, const int* exclude, int E, int ld_ex, const int* t_off, const int* t_news, long n_target, int* ahead,
                   float* t_score, int* pool_size, void* workspace, long workspace_bytes, hipStream_t stream) {
  if (!user || !reps || !pool_size || !t_off) return NNR_ERR_ARG;
  if (n_user < 1 || n_reps < 1 || D < 1 || ldu < D || ldr < D || E < 0 || ld_ex < E || (E > 0 && !exclude) || n_target < 0) return NNR_ERR_ARG;
  if (n_target > 0 && (!t_news || !ahead || !t_score)) return NNR_ERR_ARG;
  if (n_user >= INT_MAX || n_reps > INT_MAX || n_target > INT_MAX || (ARCH && ar.A > 16)) return NNR_ERR_UNSUPPORTED;
  const int splits = topk_splits(n_user, n_reps);
  const size_t need = nnr_pool_rank_workspace_bytes(n_user, n_reps, n_target);
  if (need > 0 && (!workspace || workspace_bytes < 0 || (size_t)workspace_bytes < need || ((uintptr_t)workspace & 3))) return NNR_ERR_ARG;
  const long user_tiles = (n_user + TK_TU - 1) / TK_TU;
  if (user_tiles * splits > INT_MAX) return NNR_ERR_UNSUPPORTED;
  if (!exclude) E = 0;
  if (n_target > 0) {
    hipLaunchKernelGGL(pool_rank_target_kernel<ARCH>, dim3((unsigned)((n_target + 255) / 256)), dim3(256), 0, stream, user, n_user, ldu, reps,
                       n_reps, ldr, D, valid, exclude, E, ld_ex, t_off, t_news, n_target, ahead, t_score, ar);
    NNR_CHECK_LAUNCH();
  }
  int* ws = reinterpret_cast<int*>(workspace);
  int* cnt_t = splits > 1 ? ws : ahead;
  int* cnt_u = splits > 1 ? ws + (size_t)n_target * splits : pool_size;
  const bool vec = D % 4 == 0 && ldu % 4 == 0 && ldr % 4 == 0 && al16(user) && al16(reps) && (!ARCH || ar.lda % 4 == 0);
  const dim3 grid((unsigned)(user_tiles * splits));
  if (vec)
    hipLaunchKernelGGL((pool_rank_tile_kernel<true, ARCH>), grid, dim3(256), 0, stream, user, n_user, ldu, reps, n_reps, ldr, D, valid, exclude, E,
                       ld_ex, user_tiles, splits, t_off, t_news, t_score, n_target, cnt_t, cnt_u, ar);
  else
    hipLaunchKernelGGL((pool_rank_tile_kernel<false, ARCH>), grid, dim3(256), 0, stream, user, n_user, ldu, reps, n_reps, ldr, D, valid, exclude, E,
                       ld_ex, user_tiles, splits, t_off, t_news, t_score, n_target, cnt_t, cnt_u, ar);
  NNR_CHECK_LAUNCH();
  if (splits > 1) {
    hipLaunchKernelGGL(pool_rank_merge_kernel, dim3((unsigned)((n_target + n_user + 255) / 256)), dim3(256), 0, stream, ws, n_target, n_user,
                       splits, ahead, pool_size);
    NNR_CHECK_LAUNCH();
  }
  return NNR_OK;
}

// The body of nnr_topk_scores (ARCH = false) and of nnr_topk_archive_scores
template <bool ARCH>
int topk_run(const float* user, long n_user, int ldu, const Archives& ar, const float* reps, long n_reps, int ldr, int D, const uint8_t* valid,
             const int* exclude, int E, int ld_ex, int K, int* idx, float* score, void* workspace, long workspace_bytes, hipStream_t stream) {
  if (!user || !reps || !idx || !score) return NNR_ERR_ARG;
  if (n_user < 1 || n_reps < 1 || D < 1 || ldu < D || ldr < D || E < 0 || ld_ex < E || (E > 0 && !exclude) || K < 1) return NNR_ERR_ARG;
  if (K > 64 || n_reps > INT_MAX || (ARCH && ar.A > 16)) return NNR_ERR_UNSUPPORTED;
  const int splits = topk_splits(n_user, n_reps);
  const size_t need = nnr_topk_workspace_bytes(n_user, n_reps, K);
  if (need > 0 && (!workspace || workspace_bytes < 0 || (size_t)workspace_bytes < need || ((uintptr_t)workspace & 3))) return NNR_ERR_ARG;
  const long user_tiles = (n_user + TK_TU - 1) / TK_TU;
  if (user_tiles * splits > INT_MAX || (n_user + 3) / 4 > INT_MAX) return NNR_ERR_UNSUPPORTED;
  float* ws_score = reinterpret_cast<float*>(workspace);
  int* ws_idx = reinterpret_cast<int*>(ws_score + (size_t)n_user * splits * K);
  int* t_idx = splits > 1 ? ws_idx : idx;
  float* t_score = splits > 1 ? ws_score : score;
  if (!exclude) E = 0;
  const bool vec = D % 4 == 0 && ldu % 4 == 0 && ldr % 4 == 0 && al16(user) && al16(reps) && (!ARCH || ar.lda % 4 == 0);
  const dim3 grid((unsigned)(user_tiles * splits));
  if (vec)
    hipLaunchKernelGGL((topk_tile_kernel<true, ARCH>), grid, dim3(256), 0, stream, user, n_user, ldu, reps, n_reps, ldr, D, valid, exclude, E, ld_ex,
                       K, user_tiles, splits, t_idx, t_score, ar);
  else
    hipLaunchKernelGGL((topk_tile_kernel<false, ARCH>), grid, dim3(256), 0, stream, user, n_user, ldu, reps, n_reps, ldr, D, valid, exclude, E, ld_ex,
                       K, user_tiles, splits, t_idx, t_score, ar);
  NNR_CHECK_LAUNCH();
  if (splits > 1) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((n_user + 3) / 4)), dim3(256), 0, stream, ws_score, ws_idx, n_user, splits, K, idx,
                       score);
    NNR_CHECK_LAUNCH();
  }
  return NNR_OK;
}
}  // namespace

extern "C" int nnr_pool_ranks(const float* user, long n_user, int ldu, const float* reps, long n_reps, int ldr, int D, const uint8_t* valid,
                              const int* exclude, int E, int ld_ex, const int* t_off, const int* t_news, long n_target, int* ahead,
                              float* t_score, int* pool_size, void* workspace, long workspace_bytes, hipStream_t stream) {
  return pool_ranks_run<false>(user, n_user, ldu, Archives{1, 0, 0.f}, reps, n_reps, ldr, D, valid, exclude, E, ld_ex, t_off, t_news, n_target,
                               ahead, t_score, pool_size, workspace, workspace_bytes, stream);
}

extern "C" int nnr_pool_archive_ranks(const float* user, long n_user, int ldu, int A, int lda, float scale, const float* reps, long n_reps,
                                      int ldr, int D, const uint8_t* valid, const int* exclude, int E, int ld_ex, const int* t_off,
                                      const int* t_news, long n_target, int* ahead, float* t_score, int* pool_size, void* workspace,
                                      long workspace_bytes, hipStream_t stream) {
  if (!archives_ok(ldu, A, lda, scale, D)) return NNR_ERR_ARG;
  return pool_ranks_run<true>(user, n_user, ldu, Archives{A, lda, scale}, reps, n_reps, ldr, D, valid, exclude, E, ld_ex, t_off, t_news, n_target,
                              ahead, t_score, pool_size, workspace, workspace_bytes, stream);
}

extern "C" int nnr_topk_scores(const float* user, long n_user, int ldu, const float* reps, long n_reps, int ldr, int D, const uint8_t* valid,
                               const int* exclude, int E, int ld_ex, int K, int* idx, float* score, void* workspace, long workspace_bytes,
                               hipStream_t stream) {
  return topk_run<false>(user, n_user, ldu, Archives{1, 0, 0.f}, reps, n_reps, ldr, D, valid, exclude, E, ld_ex, K, idx, score, workspace,
                         workspace_bytes, stream);
}

extern "C" int nnr_topk_archive_scores(const float* user, long n_user, int ldu, int A, int lda, float scale, const float* reps, long n_reps,
                                       int ldr, int D, const uint8_t* valid, const int* exclude, int E, int ld_ex, int K, int* idx, float* score,
                                       void* workspace, long workspace_bytes, hipStream_t stream) {
  if (!archives_ok(ldu, A, lda, scale, D)) return NNR_ERR_ARG;
  return topk_run<true>(user, n_user, ldu, Archives{A, lda, scale}, reps, n_reps, ldr, D, valid, exclude, E, ld_ex, K, idx, score, workspace,
                        workspace_bytes, stream);
}
