// Bit-reproducible table gradient from a list of occurrences SORTED BY WORD ID (nnr_token_sort, csrc/sort.hip: stable, so a word's
// occurrences keep their list order; entries without a word carry the pad key V and sort to the end):
//   dtable[w, :] += sum, in list order, of addend(occurrence) over the occurrences of w.
// Included by csrc/sort.hip, csrc/bag.hip and csrc/dssm.hip only; they differ in what an occurrence is and what it adds (a functor,
// below), not in anything stated here.
//   * Geometry.  The sorted list of `cap` entries is cut into chunks of CH (<= 64); a lane owns columns lane + 64 j, j < MAXJ (dim <=
//     64 MAXJ).  Both passes run 4 chunks per workgroup of 4 waves: grid = ceil(ceil(cap / CH) / 4) x 256 threads.
//   * Pass 1 (pass1): one wave per chunk.  It walks the chunk in list order, FL gradient rows in flight, and sums every run of equal
//     keys in registers.  A run that neither continues from the previous chunk (open_left: it is the chunk's first run and the entry
//     before the chunk has its key) nor into the next (open_right: it is the last run and the entry after the chunk has its key) is
//     the word's whole segment and is added to the table row by this wave.  Any other run is stored as a partial row of 64 MAXJ
//     floats in slot 2 c + (first run of chunk c ? 0 : 1): a chunk has at most two open runs, its first and its last, and a run that
//     is both is the first.  A chunk that reaches a pad key stops there; its last run is closed.
//   * Pass 2 (fix): a workgroup looks after its 4 chunks in order.  A chunk OWNS a run that starts in it and continues into the next:
//     its first run if the entry before the chunk differs and the chunk's last entry and the entry after it have the same key, else
//     its last run if the entry after the chunk has that key.  For an owned run the waves add slot 0 of the following chunks that
//     begin with the key, found 64 chunks per ballot: in each window wave w takes chunks w, w + 4, ... in ascending order (U rows in
//     flight), a wave keeps its sum across windows, and wave 0 writes (((own slot + sum 0) + sum 1) + sum 2) + sum 3.  A frequent
//     word's segment is hundreds of chunks long (the top word of a Zipf vocabulary owns a seventh of the tokens): one wave walking it
//     alone was the kernel's long pole.
//   * Order and writers.  Every addition above has a fixed order, so the same list gives the same bits.  A table row is written
//     exactly once per launch pair: by pass 1 if its segment lies inside one chunk, else by the fix pass of the chunk that owns it.
//     ATOMIC = false writes it with a plain read-add-write.  ATOMIC = true uses one atomicAdd per element, for a table gradient that
//     other streams add to during the same step: two addends into a zeroed buffer commute, so that stays reproducible too.
//   * Traffic: every occurrence's gradient row is read once, every touched table row written once, + 2 x 256 MAXJ bytes per
//     chunk-crossing run.  Workspace: two slots per chunk (ws_floats); nothing is read that was not written in the same call.
// The functor F of pass 1 supplies
//   struct Rec            what a lane knows about its sorted entry: 32-bit fields only, broadcast word by word with __shfl
//   Rec pad()             the record of a lane without an entry; its rows must be readable (they are loaded and discarded)
//   Rec record(p, live)   the record of sorted entry p; live = false: p carries the pad key
//   NV, nv()              rows loaded per occurrence: at most NV, nv() (wave-uniform) in this launch
//   row(rec, k)           row k < nv() of the occurrence: `dim` floats
//   prep(rec)             what the occurrence's addends share, computed once per occurrence (the record itself if nothing)
//   addend(pre, col, in, x)   what the occurrence adds at column col from the loaded x[k < nv()]; in = col < dim, x is a clamped
//                         column's value otherwise
#pragma once
#include "common.h"

namespace sorted_rows {

constexpr size_t ws_floats(long cap, int CH, int MAXJ) { return cap <= 0 ? 0 : (size_t)((cap + CH - 1) / CH) * 2 * 64 * MAXJ; }
static inline unsigned blocks(long cap, int CH) { return (unsigned)(((cap + CH - 1) / CH + 3) / 4); }

template <bool ATOMIC> __device__ __forceinline__ void add(float* p, float x) {
  if constexpr (ATOMIC) atomicAdd(p, x);
  else *p += x;
}

template <class Rec> __device__ __forceinline__ Rec bcast(const Rec& r, int i) {
  static_assert(sizeof(Rec) % 4 == 0, "32-bit fields only");
  uint32_t w[sizeof(Rec) / 4];
  __builtin_memcpy(w, &r, sizeof(Rec));
#pragma unroll
  for (unsigned k = 0; k < sizeof(Rec) / 4; ++k) w[k] = __shfl(w[k], i, 64);
  Rec o;
  __builtin_memcpy(&o, w, sizeof(Rec));
  return o;
}

// TAIL_TEST: row i of a short last chunk gets the pad key from a scalar test of i against the chunk's count, not from the shuffle.  The
// result is the same (lanes >= cnt hold the pad key); it is measured 3 % faster at CH 64 / FL 4 and 4 % slower at CH 32 / FL 8
// (profiles/sorted_rows_ab.md), so an instance says which it wants.
template <int CH, int MAXJ, int FL, bool ATOMIC, bool TAIL_TEST, class F>
__device__ __forceinline__ void pass1(const F& f, const unsigned* keys, long cap, unsigned V, int dim, float* dtable,
                                      float* partial) {
  typedef typename F::Rec Rec;
  constexpr int PITCH = 64 * MAXJ;
  static_assert(CH <= 64 && CH % FL == 0, "a chunk is one wave's lanes, walked FL at a time");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long c = blockIdx.x * 4L + wv;
  const long p0 = c * CH;
  if (p0 >= cap) return;
  const long p1 = min(cap, p0 + CH);
  const int cnt = (int)(p1 - p0);
  unsigned myk = V;
  Rec mine = f.pad();
  if (lane < cnt) {
    myk = keys[p0 + lane];
    mine = f.record(p0 + lane, myk < V);
  }
  const unsigned k0 = __shfl(myk, 0, 64);
  if (k0 >= V) return;                                            // sorted: nothing but pad entries from here on
  const unsigned prevK = p0 > 0 ? keys[p0 - 1] : 0xFFFFFFFFu;     // (0xFFFFFFFF equals no valid key)
  const unsigned nextK = p1 < cap ? keys[p1] : 0xFFFFFFFFu;
  float acc[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
  unsigned run_key = k0;
  bool first = true;
  auto flush = [&](bool open_right) {
    const bool open_left = first && prevK == run_key;
    if (!open_left && !open_right) {                              // the whole segment of this word: this wave is the row's only writer
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int col = lane + 64 * j;
        if (col < dim) add<ATOMIC>(&dtable[(long)run_key * dim + col], acc[j]);
      }
    } else {
      float* dst = partial + (c * 2 + (first ? 0 : 1)) * (long)PITCH;
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) dst[lane + 64 * j] = acc[j];
    }
  };
  bool done = false;
  const int dlast = dim - 1;
  const int nv = f.nv();
  for (int i0 = 0; i0 < cnt && !done; i0 += FL) {
    // FL rows in flight: every load is issued UNCONDITIONALLY before any of them is used (a branch per row cuts the block, and the
    // wait for row u's loads then sits in front of row u + 1's: one row in flight -- 32 dependent round trips per wave, 85 us for an
    // 88 k-row stream); pad entries read the pad record's rows / a clamped column and are discarded below
    float v[FL][MAXJ][F::NV];
    unsigned kk[FL];
    Rec rec[FL];
#pragma unroll
    for (int u = 0; u < FL; ++u) {
      const int i = i0 + u;                                       // (< CH <= 64: lanes >= cnt hold the pad key and the pad record)
      kk[u] = (!TAIL_TEST || i < cnt) ? __shfl(myk, i, 64) : V;
      rec[u] = bcast(mine, i);
    }
#pragma unroll
    for (int u = 0; u < FL; ++u) {
#pragma unroll
      for (int k = 0; k < F::NV; ++k) {
        if (k < nv) {
          const float* src = f.row(rec[u], k);
#pragma unroll
          for (int j = 0; j < MAXJ; ++j) v[u][j][k] = src[min(lane + 64 * j, dlast)];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < FL; ++u) {
      if (done) break;
      if (kk[u] >= V) { done = true; break; }
      if (kk[u] != run_key) {
        flush(false);
        run_key = kk[u];
        first = false;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
      }
      const auto pre = f.prep(rec[u]);
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int col = lane + 64 * j;
        acc[j] += f.addend(pre, col, col < dim, v[u][j]);
      }
    }
  }
  flush(nextK == run_key);                                        // (a chunk that ran into pad entries has nextK = pad: closed)
}

template <int CH, int MAXJ, int U, bool ATOMIC>
__device__ __forceinline__ void fix(const unsigned* keys, long cap, unsigned V, int dim, float* dtable,
                                    const float* partial) {
  constexpr int PITCH = 64 * MAXJ;
  __shared__ float red[4][PITCH];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: so are the partial rows' addresses)
  const long nchunks = (cap + CH - 1) / CH;
  for (int ci = 0; ci < 4; ++ci) {
    const long c = blockIdx.x * 4L + ci;
    const long p0 = c * CH;
    if (p0 >= cap) break;                                          // (uniform over the workgroup, like every branch below)
    const long p1 = min(cap, p0 + CH);
    const unsigned k0 = keys[p0];
    if (k0 >= V) break;                                            // sorted: nothing but pad entries from here on
    const unsigned prevK = p0 > 0 ? keys[p0 - 1] : 0xFFFFFFFFu;
    const unsigned kl = keys[p1 - 1];
    const unsigned nextK = p1 < cap ? keys[p1] : 0xFFFFFFFFu;
    for (int cand = 0; cand < 2; ++cand) {
      // cand 0: the chunk's first run, if the segment STARTS here and runs on into the next chunk; cand 1: its last run, likewise
      const unsigned key = cand == 0 ? k0 : kl;
      const bool own = cand == 0 ? (prevK != k0 && kl == k0 && nextK == k0) : (kl != k0 && kl < V && nextK == kl);
      if (!own) continue;
      float acc[MAXJ];
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
      long cc = c + 1;
      while (true) {
        const bool cont = (cc + lane < nchunks) && keys[(cc + lane) * CH] == key;
        const unsigned long long m = __ballot(cont);
        const int nc = (m == ~0ull) ? 64 : __builtin_ctzll(~m);   // chunks cc .. cc + nc - 1 begin with this word: their slot 0 is its partial
        for (int q = wv; q < nc; q += 4 * U) {                     // this wave: chunks q, q + 4, ... of the window, in order
          float v[U][MAXJ];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float* sp = partial + ((cc + min(q + 4 * u, nc - 1)) * 2) * (long)PITCH;
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) v[u][j] = sp[lane + 64 * j];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (q + 4 * u < nc) {
#pragma unroll
              for (int j = 0; j < MAXJ; ++j) acc[j] += v[u][j];
            }
          }
        }
        cc += nc;
        if (nc < 64) break;
      }
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) red[wv][lane + 64 * j] = acc[j];
      __syncthreads();
      if (wv == 0) {
        const float* src = partial + (c * 2 + cand) * (long)PITCH;        // the run's own part in its first chunk
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
          const int col = lane + 64 * j;
          const float t = (((src[col] + red[0][col]) + red[1][col]) + red[2][col]) + red[3][col];
          if (col < dim) add<ATOMIC>(&dtable[(long)key * dim + col], t);
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace sorted_rows
