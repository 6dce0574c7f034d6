// Data side of the hot path, device resident.
//
// * corpus_batch_kernel : MIND_Train_Dataset.__getitem__ + default collate (MIND_dataset.py:70-76) as ONE gather kernel over
//   corpus tables that live in HBM: a batch is described by behaviour indices + (1 + K) sampled news ids per behaviour
//   (a few hundred bytes over PCIe instead of 98.6 KB per impression), one wave per news slot, one per impression for the
//   per-behaviour fields.  HBM-bound byte work: 1.45 KB read + 1.45 KB written per news slot (T = 32, C = 128).
// * history_graph_kernel : the per-behaviour user-history graph, cluster mask and cluster indices that the reference
//   pre-computes into a [behaviours, G, G] fp32 array (MIND_corpus.py:162-221; 18.5 KB per behaviour line, tens of GB of
//   host memory on MIND-large) built on the fly from the history's category ids: one workgroup per impression, the
//   G x G adjacency assembled in LDS, normalised with correctly rounded fp32 div / sqrt / mul (no contraction) so the result is
//   bit-identical to numpy's, written once (18.5 KB).
// * negative_sample_kernel : the epoch's (1 + K) sampled news ids per behaviour (MIND_dataset.py:27-47) as a pure function of
//   (seed, epoch, behaviour), written in place into the table corpus_batch_kernel reads.
// * list_scores_kernel : the click scores of a whole evaluation as one gather (listwise evaluation): sample j's score is the dot product
//   of row row[j] of the user table and row cand[j] of the news table, one wave per sample.
// * cne_pair_triples_kernel : the pairing plan of de-duplicated evaluation: for every encoder call of a range of reference batches, the news
//   whose memories gate each sequence of the call under CNE's rank pairing -- a stable counting sort per call, integers only.
#include "common.h"

namespace {

struct CorpusTables {
  const int* news_category; const int* news_subCategory;
  const int* title_text; const uint8_t* title_mask; const int* title_entity;
  const int* abstract_text; const uint8_t* abstract_mask; const int* abstract_entity;
  const long* beh_user; const int* beh_history; const uint8_t* beh_history_mask; const int* beh_line;
  const float* graph_table; const uint8_t* cmask_table; const long* cidx_table;    // optional pre-built graphs (else null)
  int T, C, H, G, K1;
};
struct BatchOut {
  long* user_id;
  int* u_cat; int* u_sub; int* u_tt; uint8_t* u_tm; int* u_te; int* u_ct; uint8_t* u_cm; int* u_ce;
  uint8_t* u_hmask; float* u_graph; uint8_t* u_cmask; long* u_cidx;
  int* n_cat; int* n_sub; int* n_tt; uint8_t* n_tm; int* n_te; int* n_ct; uint8_t* n_cm; int* n_ce;
};

template <typename T>
__device__ __forceinline__ void copy_row(T* dst, const T* src, int n, int lane) {
  for (int i = lane; i < n; i += 64) dst[i] = src[i];
}

// grid = B * (H + S) news slots + B per-impression slots; block = one wave
__global__ __launch_bounds__(64) void corpus_batch_kernel(CorpusTables t, BatchOut o, const int* __restrict__ beh_idx,
                                                          const int* __restrict__ samples, int ld_samples, int B, int S) {
  const int lane = threadIdx.x;
  const int slots = B * (t.H + S);
  const int bid = blockIdx.x;
  if (bid < slots) {
    const int b = bid / (t.H + S), k = bid - b * (t.H + S);
    const int beh = beh_idx[b];
    const bool hist = k < t.H;
    const int news = hist ? t.beh_history[(long)beh * t.H + k] : samples[(long)beh * ld_samples + (k - t.H)];
    const long dst = hist ? (long)b * t.H + k : (long)b * S + (k - t.H);
    int* cat = hist ? o.u_cat : o.n_cat; int* sub = hist ? o.u_sub : o.n_sub;
    int* tt = hist ? o.u_tt : o.n_tt; uint8_t* tm = hist ? o.u_tm : o.n_tm; int* te = hist ? o.u_te : o.n_te;
    int* ct = hist ? o.u_ct : o.n_ct; uint8_t* cm = hist ? o.u_cm : o.n_cm; int* ce = hist ? o.u_ce : o.n_ce;
    if (lane == 0) { cat[dst] = t.news_category[news]; sub[dst] = t.news_subCategory[news]; }
    copy_row(tt + dst * t.T, t.title_text + (long)news * t.T, t.T, lane);
    copy_row(te + dst * t.T, t.title_entity + (long)news * t.T, t.T, lane);
    copy_row(ct + dst * t.C, t.abstract_text + (long)news * t.C, t.C, lane);
    copy_row(ce + dst * t.C, t.abstract_entity + (long)news * t.C, t.C, lane);
    if (((t.T | t.C) & 3) == 0) {      // mask rows are whole dwords
      copy_row(reinterpret_cast<uint32_t*>(tm + dst * t.T), reinterpret_cast<const uint32_t*>(t.title_mask + (long)news * t.T), t.T >> 2, lane);
      copy_row(reinterpret_cast<uint32_t*>(cm + dst * t.C), reinterpret_cast<const uint32_t*>(t.abstract_mask + (long)news * t.C), t.C >> 2, lane);
    } else {
      copy_row(tm + dst * t.T, t.title_mask + (long)news * t.T, t.T, lane);
      copy_row(cm + dst * t.C, t.abstract_mask + (long)news * t.C, t.C, lane);
    }
    return;
  }
  const int b = bid - slots;
  if (b >= B) return;
  const int beh = beh_idx[b];
  if (lane == 0) o.user_id[b] = t.beh_user[beh];
  copy_row(o.u_hmask + (long)b * t.H, t.beh_history_mask + (long)beh * t.H, t.H, lane);
  if (t.graph_table) {               // pre-built graphs resident in HBM (the reference's layout): plain row gather
    const int line = t.beh_line[beh];
    copy_row(o.u_graph + (long)b * t.G * t.G, t.graph_table + (long)line * t.G * t.G, t.G * t.G, lane);
    copy_row(o.u_cmask + (long)b * t.K1, t.cmask_table + (long)line * t.K1, t.K1, lane);
    copy_row(o.u_cidx + (long)b * t.H, t.cidx_table + (long)line * t.H, t.H, lane);
  }
}

constexpr int GMAX = 96;
// cats [B, H] : category of every history slot (the batch's user_category); hmask [B, H] : slot is real history
__global__ __launch_bounds__(256) void history_graph_kernel(const int* __restrict__ cats, const uint8_t* __restrict__ hmask, int B, int H,
                                                            int K, int norm, float* __restrict__ graph, uint8_t* __restrict__ cmask,
                                                            long* __restrict__ cidx) {
  __shared__ float A[GMAX * GMAX];
  __shared__ float dsc[GMAX];
  __shared__ int cat[GMAX];
  __shared__ int nh;
  const int b = blockIdx.x, tid = threadIdx.x, G = H + K;
  if (tid == 0) nh = 0;
  __syncthreads();
  for (int i = tid; i < H; i += 256) {
    cat[i] = cats[(long)b * H + i];
    if (hmask[(long)b * H + i]) atomicAdd(&nh, 1);        // the mask is a prefix (MIND_corpus.py:352-353): count = history length
  }
  const float diag = norm == 3 ? 0.f : 1.f;                                                  // :180-183 --no_self_connection: zero diagonal
  for (int i = tid; i < G * G; i += 256) A[i] = ((i / G) == (i % G)) ? diag : 0.f;           // :183 identity (self connections)
  __syncthreads();
  const int n = nh;
  for (int i = tid; i < K + 1; i += 256) cmask[(long)b * (K + 1) + i] = 0;
  for (int i = tid; i < H; i += 256) cidx[(long)b * H + i] = (i < n) ? (long)cat[i] : (long)K;   // :185,:192
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int c = cat[i];
    cmask[(long)b * (K + 1) + c] = 1;                                                        // :191 (same value from every writer)
    A[i * G + H + c] = 1.f;                                                                  // :194-195
    A[(H + c) * G + i] = 1.f;
  }
  for (int p = tid; p < n * n; p += 256) {
    const int i = p / n, j = p - i * n;
    if (j <= i) continue;
    const int ci = cat[i], cj = cat[j];
    if (ci == cj) { A[i * G + j] = 1.f; A[j * G + i] = 1.f; }                                // :199-200
    else { A[(H + ci) * G + H + cj] = 1.f; A[(H + cj) * G + H + ci] = 1.f; }                // :202-203
  }
  __syncthreads();
  float* out = graph + (long)b * G * G;
  if (n == 0 || norm == 0 || norm == 3) {                                                                 // :186 empty history stays un-normalised
    for (int i = tid; i < G * G; i += 256) out[i] = A[i];
    return;
  }
  for (int i = tid; i < G; i += 256) {
    float sm = 0.f;
    for (int j = 0; j < G; ++j) sm += A[i * G + j];                                          // small integers: exact
    // plain `/` and sqrtf are correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (the
    // __fdiv_rn / __fsqrt_rn intrinsics map to the 1-ulp native instructions and differed from numpy in 0.9 % of entries)
    const float inv = 1.f / sm;
    dsc[i] = (norm == 2) ? inv : sqrtf(inv);                                                 // :207 / :212
  }
  __syncthreads();
  for (int p = tid; p < G * G; p += 256) {
    const int i = p / G, j = p - i * G;
    const float v = __fmul_rn(dsc[i], A[p]);
    out[p] = (norm == 2) ? v : __fmul_rn(v, dsc[j]);                                         // :209 / :214
  }
}

}  // namespace

extern "C" int nnr_corpus_batch(const nnr_corpus_tables* t, const nnr_batch_out* o, const int* beh_idx, const int* samples, int ld_samples,
                                int B, int S, hipStream_t stream) {
  if (!t || !o || !beh_idx || !samples || B <= 0 || S <= 0) return NNR_ERR_ARG;
  CorpusTables ct;
  ct.news_category = t->news_category; ct.news_subCategory = t->news_subCategory; ct.title_text = t->title_text;
  ct.title_mask = t->title_mask; ct.title_entity = t->title_entity; ct.abstract_text = t->abstract_text;
  ct.abstract_mask = t->abstract_mask; ct.abstract_entity = t->abstract_entity; ct.beh_user = t->beh_user;
  ct.beh_history = t->beh_history; ct.beh_history_mask = t->beh_history_mask; ct.beh_line = t->beh_line;
  ct.graph_table = t->graph_table; ct.cmask_table = t->cmask_table; ct.cidx_table = t->cidx_table;
  ct.T = t->T; ct.C = t->C; ct.H = t->H; ct.G = t->G; ct.K1 = t->K1;
  if (ct.graph_table && (!ct.cmask_table || !ct.cidx_table || !ct.beh_line)) return NNR_ERR_ARG;
  BatchOut bo;
  bo.user_id = o->user_id; bo.u_cat = o->u_cat; bo.u_sub = o->u_sub; bo.u_tt = o->u_tt; bo.u_tm = o->u_tm; bo.u_te = o->u_te;
  bo.u_ct = o->u_ct; bo.u_cm = o->u_cm; bo.u_ce = o->u_ce; bo.u_hmask = o->u_hmask; bo.u_graph = o->u_graph; bo.u_cmask = o->u_cmask;
  bo.u_cidx = o->u_cidx; bo.n_cat = o->n_cat; bo.n_sub = o->n_sub; bo.n_tt = o->n_tt; bo.n_tm = o->n_tm; bo.n_te = o->n_te;
  bo.n_ct = o->n_ct; bo.n_cm = o->n_cm; bo.n_ce = o->n_ce;
  hipLaunchKernelGGL(corpus_batch_kernel, dim3(B * (ct.H + S) + B), dim3(64), 0, stream, ct, bo, beh_idx, samples, ld_samples, B, S);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

extern "C" int nnr_history_graph(const int* cats, const uint8_t* hmask, int B, int H, int K, int norm, float* graph, uint8_t* cmask,
                                 long* cidx, hipStream_t stream) {
  if (!cats || !hmask || !graph || !cmask || !cidx || B <= 0) return NNR_ERR_ARG;
  if (H + K > GMAX || norm < 0 || norm > 3) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(history_graph_kernel, dim3(B), dim3(256), 0, stream, cats, hmask, B, H, K, norm, graph, cmask, cidx);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

// ------------------------------------------------------------------------------------------------ negative sampling (f-1)
// MIND_Train_Dataset.negative_sampling (MIND_dataset.py:27-47) on the device: one thread per behaviour, a few hundred bytes per row.
// The construction (generator, mapping, walk) is written down once, at nnr_negative_sample in include/nnr_hip.h.
namespace {
constexpr int NEG_KMAX = 16;

// every loop is bounded by NEG_KMAX (no rejection loop); all register indices are static after unrolling: no scratch
__global__ __launch_bounds__(256) void negative_sample_kernel(const int* __restrict__ clicks, const long* __restrict__ neg_offsets,
                                                              const int* __restrict__ neg_ids, const int* __restrict__ beh_idx, int n, int K,
                                                              uint32_t seed, int epoch, int* __restrict__ samples, int ld_samples) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int beh = beh_idx ? beh_idx[i] : i;
  const long off = neg_offsets[beh];
  const long len = neg_offsets[beh + 1] - off;
  if (len <= 0 || len > 0x7fffffffL) return;             // refused on the host when the lists are uploaded
  const int* __restrict__ list = neg_ids + off;
  int* __restrict__ row = samples + (long)beh * ld_samples;
  row[0] = clicks[beh];
  const uint32_t m = (uint32_t)len;
  if (m <= (uint32_t)K) {                                  // cyclic fill, exact
    for (int j = 0; j < K; ++j) row[j + 1] = list[(uint32_t)j % m];
    return;
  }
  // partial Fisher-Yates over the virtual array a[p] = p: (pos[t], val[t]) is the one entry step t displaced, pos[t] < 0: none
  const uint32_t key = nnr_hash32(seed ^ nnr_hash32((uint32_t)epoch + 0x9E3779B9u));
  const uint32_t h = nnr_hash32((uint32_t)beh ^ key);
  int pos[NEG_KMAX], val[NEG_KMAX];
#pragma unroll
  for (int j = 0; j < NEG_KMAX; ++j) {
    if (j >= K) break;
    const uint32_t r = nnr_hash32(h + (uint32_t)j * 0x9E3779B9u + 1u);
    const int p = j + (int)(((uint64_t)r * (uint64_t)(m - (uint32_t)j)) >> 32);       // uniform in [j, m)
    int ap = p, aj = j, hit = -1;
#pragma unroll
    for (int t = 0; t < j; ++t) {
      if (pos[t] == p) { ap = val[t]; hit = t; }
      if (pos[t] == j) aj = val[t];
    }
#pragma unroll
    for (int t = 0; t < j; ++t)
      if (t == hit) val[t] = aj;                           // a[p] = a[j]; position j itself is never read again
    pos[j] = hit < 0 ? p : -1;
    val[j] = aj;
    row[j + 1] = list[ap];
  }
}
}  // namespace

extern "C" int nnr_negative_sample(const int* clicks, const long* neg_offsets, const int* neg_ids, const int* beh_idx, int n, int K,
                                   uint32_t seed, int epoch, int* samples, int ld_samples, hipStream_t stream) {
  if (!clicks || !neg_offsets || !neg_ids || !samples || n <= 0) return NNR_ERR_ARG;
  if (K < 1 || K > NEG_KMAX) return NNR_ERR_UNSUPPORTED;
  if (ld_samples < 1 + K) return NNR_ERR_ARG;
  hipLaunchKernelGGL(negative_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, clicks, neg_offsets, neg_ids, beh_idx, n, K, seed,
                     epoch, samples, ld_samples);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

// ------------------------------------------------------------------------------------------------ ranking metrics (f-4)
// The tail of util.compute_scores (util.py:50-59) and evaluate.scoring (evaluate.py:32-89) on the device: one workgroup per
// impression ranks its candidates by descending score (equal scores keep file order, like Python's stable sort) and
// evaluates AUC (roc_auc_score on 1/rank = correctly ordered (positive, negative) pairs / all pairs), MRR, nDCG@5, nDCG@10
// in float64.  An impression with no click or only clicks has no AUC (sklearn raises): its four values are NaN.
namespace {
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void rank_metrics_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                          const long* __restrict__ offsets, int* __restrict__ ranks,
                                                          double* __restrict__ per_imp) {
  __shared__ double sh[256];
  const int imp = blockIdx.x, tid = threadIdx.x;
  const long o = offsets[imp];
  const int n = (int)(offsets[imp + 1] - o);
  const float* s = scores + o;
  const uint8_t* y = labels + o;
  double pos = 0, auc_num = 0, rr = 0, dcg5 = 0, dcg10 = 0;
  for (int i = tid; i < n; i += 256) {
    const float si = s[i];
    int better = 0, neg_below = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s[j];
      const bool before = (sj > si) || (sj == si && j < i);        // j is ranked ahead of i
      better += before;
      neg_below += (!before && j != i && !y[j]);                   // negatives ranked after i
    }
    const int rank = better + 1;
    ranks[o + i] = rank;
    if (y[i]) {
      pos += 1;
      auc_num += neg_below;
      rr += 1.0 / rank;
      const double g = 1.0 / log2((double)rank + 1.0);
      if (rank <= 5) dcg5 += g;
      if (rank <= 10) dcg10 += g;
    }
  }
  const double P = block_sum(pos, sh);
  const double A = block_sum(auc_num, sh), R = block_sum(rr, sh), D5 = block_sum(dcg5, sh), D10 = block_sum(dcg10, sh);
  if (tid == 0) {
    const double N = n - P;
    double best5 = 0, best10 = 0;
    for (int k = 0; k < 10 && k < (int)P; ++k) {
      const double g = 1.0 / log2((double)k + 2.0);
      if (k < 5) best5 += g;
      best10 += g;
    }
    const bool ok = P > 0 && N > 0;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    per_imp[4 * imp + 0] = ok ? A / (P * N) : nan;
    per_imp[4 * imp + 1] = ok ? R / P : nan;
    per_imp[4 * imp + 2] = ok ? D5 / best5 : nan;
    per_imp[4 * imp + 3] = ok ? D10 / best10 : nan;
  }
}
}  // namespace

extern "C" int nnr_rank_metrics(const float* scores, const uint8_t* labels, const long* offsets, int n_impressions, int* ranks,
                                double* per_impression, hipStream_t stream) {
  if (!scores || !labels || !offsets || !ranks || !per_impression || n_impressions <= 0) return NNR_ERR_ARG;
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(n_impressions), dim3(256), 0, stream, scores, labels, offsets, ranks, per_impression);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

// ------------------------------------------------------------------------------------------------ listwise scores
// scores[j] = <user[row[j]], reps[cand[j]]>: the click predictor of a whole dev / test split in one launch, after the user encoder ran once
// per impression (or once per row of K candidates) instead of once per sample.  One wave per sample, four per workgroup, grid-stride.  The
// summation order is the one nnr_list_scores states in include/nnr_hip.h: lane l folds d = l, l + 64, ... in ascending order with fmaf,
// wave_sum folds the lanes.  Both load paths keep it to the bit: the 16-byte path lets lane 4g + q load the float4 at 64q + 4g of each
// 256-float chunk (a wave still reads the chunk's 1 KB contiguously) and transposes the 4 x 4 block inside the quad with two DPP swaps, after
// which lane l = 4g + c holds the elements l, l + 64, l + 128, l + 192 of the chunk -- what the scalar path loads.  No LDS, no atomics.
namespace {
constexpr int LS_GRID_MAX = 2048;                          // 8 workgroups (32 waves) per CU on 256 CUs: every wave slot taken, no more

template <int CTRL> __device__ __forceinline__ float quad_perm(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// a[c] of quad lane t  ->  a[s] = (a[t] of quad lane s); every lane of the wave must be active
__device__ __forceinline__ void quad_transpose(float (&a)[4], bool b0, bool b1) {
#pragma unroll
  for (int p = 0; p < 4; p += 2) {                         // lanes t, t ^ 1 swap the off-diagonal of each 2 x 2 block
    const float got = quad_perm<0xB1>(b0 ? a[p] : a[p + 1]);      // quad_perm [1, 0, 3, 2]
    if (b0) a[p] = got; else a[p + 1] = got;
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {                            // lanes t, t ^ 2 swap the off-diagonal 2 x 2 blocks
    const float got = quad_perm<0x4E>(b1 ? a[p] : a[p + 2]);      // quad_perm [2, 3, 0, 1]
    if (b1) a[p] = got; else a[p + 2] = got;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void list_scores_kernel(const float* __restrict__ user, int ldu, const float* __restrict__ reps, int ldr,
                                                          const int* __restrict__ row, const int* __restrict__ cand, long n, int D,
                                                          float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const long step = gridDim.x * 4L;
  long j = blockIdx.x * 4L + (threadIdx.x >> 6);           // wave-uniform: a wave is wholly inside the loop or wholly out
  if (j >= n) return;
  int ru = row[j], rc = cand[j];
  while (true) {
    const float* __restrict__ u = user + (long)ru * ldu;
    const float* __restrict__ r = reps + (long)rc * ldr;
    const long jn = j + step;
    if (jn < n) { ru = row[jn]; rc = cand[jn]; }           // the next trip's indices travel under this trip's rows
    float acc = 0.f;
    if (VEC) {
      const int q = lane & 3, g = lane >> 2;
      const bool b0 = lane & 1, b1 = lane & 2;
      for (int base = 0; base < D; base += 256) {
        const int off = base + 64 * q + 4 * g;             // D % 4 == 0: a float4 is wholly inside the row or wholly outside
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
        if (off < D) {
          const float4 ua = *reinterpret_cast<const float4*>(u + off), ra = *reinterpret_cast<const float4*>(r + off);
          a[0] = ua.x; a[1] = ua.y; a[2] = ua.z; a[3] = ua.w;
          b[0] = ra.x; b[1] = ra.y; b[2] = ra.z; b[3] = ra.w;
        }
        quad_transpose(a, b0, b1);
        quad_transpose(b, b0, b1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (base + 64 * s + lane < D) acc = fmaf(a[s], b[s], acc);
      }
    } else {
      for (int d = lane; d < D; d += 64) acc = fmaf(u[d], r[d], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) scores[j] = acc;
    if (jn >= n) break;
    j = jn;
  }
}
}  // namespace

extern "C" int nnr_list_scores(const float* user, long n_user, int ldu, const float* reps, long n_reps, int ldr, const int* row,
                               const int* cand, long n, int D, float* scores, hipStream_t stream) {
  if (!user || !reps || !row || !cand || !scores) return NNR_ERR_ARG;
  if (n < 1 || D < 1 || ldu < D || ldr < D || n_user < 1 || n_reps < 1) return NNR_ERR_ARG;
  const bool vec = D % 4 == 0 && ldu % 4 == 0 && ldr % 4 == 0 && ((uintptr_t)user | (uintptr_t)reps) % 16 == 0;
  const long blocks = (n + 3) / 4;
  const dim3 grid((unsigned)(blocks < LS_GRID_MAX ? blocks : LS_GRID_MAX));
  if (vec) hipLaunchKernelGGL(list_scores_kernel<true>, grid, dim3(256), 0, stream, user, ldu, reps, ldr, row, cand, n, D, scores);
  else hipLaunchKernelGGL(list_scores_kernel<false>, grid, dim3(256), 0, stream, user, ldu, reps, ldr, row, cand, n, D, scores);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}

// ------------------------------------------------------------------------------------------------ CNE pairing plan
// De-duplicated evaluation of the rank-pairing encoders: which news gate which, for every encoder call of a range of reference batches.
// Block k < batches plans the history call of batch k (b * H sequences, sequence s * H + h = beh_history[s, h]: contiguous in memory),
// block batches + k its candidate call (b sequences).  Wave 0 ranks the call by title length, wave 1 by content length: a counting sort
// over 256 length bins in LDS, three passes of 64 sequences per trip in ascending sequence order --
//   count    bin[l] = sequences of length l                       (the first lane of every group of equal lengths adds the group's size)
//   starts   bin[l] = sequences longer than l                     (descending order: a suffix sum, four bins per lane + a shuffle scan)
//   place    position = bin[l] + equal lengths in lower lanes;    bin[l] += the group's size
// -- so equal lengths keep their sequence order: torch.sort(descending=True, stable=True).  A group is found with one ballot per length
// bit; one lane per bin touches the bin and a wave's LDS operations complete in order, so there are no atomics anywhere.  The wave leaves
// rank[i] in its output row and the news in sorted order in the workspace; after the barrier sequence i picks news_sorted_c[rank_t[i]]
// and news_sorted_t[rank_c[i]].  Integers only: the same bits on every run.
namespace {
constexpr int PT_BINS = 256;

// the valid lanes of this trip whose length equals this lane's
__device__ __forceinline__ uint64_t same_length_lanes(int l, bool valid) {
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (l >> b) & 1;
    const uint64_t m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}

__global__ __launch_bounds__(128) void cne_pair_triples_kernel(const int* __restrict__ hist, const int* __restrict__ cand,
                                                               const int* __restrict__ tlen, const int* __restrict__ clen, int H, int n_news,
                                                               int batch_size, long first, long count, int* pc_hist, int* pt_hist,
                                                               int* pc_cand, int* pt_cand, int* tmp) {
  __shared__ int bins[2][PT_BINS];
  const int x = threadIdx.x >> 6, lane = threadIdx.x & 63;          // wave 0: the title stream, wave 1: the content stream
  const long batches = (count + batch_size - 1) / batch_size;
  const bool is_cand = (long)blockIdx.x >= batches;
  const long k = is_cand ? (long)blockIdx.x - batches : (long)blockIdx.x;
  const long s0 = k * batch_size;                                    // the call's first sample, counted from `first`
  if (s0 >= count) return;                                           // (block-uniform; the grid is exactly 2 * batches)
  const int b = (int)(count - s0 < (long)batch_size ? count - s0 : (long)batch_size);
  const int m = is_cand ? b : b * H;                                 // sequences of the call
  const int* __restrict__ ids = is_cand ? cand + first + s0 : hist + (first + s0) * H;
  const long o = is_cand ? s0 : s0 * H;
  int* pc = (is_cand ? pc_cand : pc_hist) + o;
  int* pt = (is_cand ? pt_cand : pt_hist) + o;
  int* ws = is_cand ? tmp + 2 * count * H : tmp;                     // [2][count * H] history calls, then [2][count] candidate calls
  const long stride = is_cand ? count : count * H;
  int* sorted_t = ws + o;
  int* sorted_c = ws + stride + o;

  const int* __restrict__ len = x ? clen : tlen;
  int* rank_out = x ? pt : pc;                                       // rank_t waits in pc's row, rank_c in pt's
  int* sorted = x ? sorted_c : sorted_t;
  volatile int* bin = bins[x];
  const uint64_t lower = (1ull << lane) - 1ull;

  for (int q = lane; q < PT_BINS; q += 64) bin[q] = 0;
  __builtin_amdgcn_wave_barrier();
  for (int base = 0; base < m; base += 64) {                         // count
    const int i = base + lane;
    const bool valid = i < m;
    int l = 0;
    if (valid) {
      const int id = ids[i];
      l = (unsigned)id < (unsigned)n_news ? len[id] : 0;
      l = l < 0 ? 0 : (l > PT_BINS - 1 ? PT_BINS - 1 : l);
    }
    const uint64_t peers = same_length_lanes(l, valid);
    if (valid && (peers & lower) == 0) bin[l] = bin[l] + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
  {                                                                  // starts: bin[l] = sequences longer than l
    int h[4], s = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) { h[u] = bin[4 * lane + u]; s += h[u]; }
    int incl = s;                                                    // this lane's bins and every higher lane's
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_down(incl, d, 64);
      if (lane + d < 64) incl += v;
    }
    const int above = incl - s;
    __builtin_amdgcn_wave_barrier();
    bin[4 * lane + 3] = above;
    bin[4 * lane + 2] = above + h[3];
    bin[4 * lane + 1] = above + h[3] + h[2];
    bin[4 * lane + 0] = above + h[3] + h[2] + h[1];
    __builtin_amdgcn_wave_barrier();
  }
  for (int base = 0; base < m; base += 64) {                         // place
    const int i = base + lane;
    const bool valid = i < m;
    int l = 0, id = 0;
    if (valid) {
      id = ids[i];
      l = (unsigned)id < (unsigned)n_news ? len[id] : 0;
      l = l < 0 ? 0 : (l > PT_BINS - 1 ? PT_BINS - 1 : l);
    }
    const uint64_t peers = same_length_lanes(l, valid);
    const int before = __popcll(peers & lower);
    int pos = 0;
    if (valid) pos = bin[l] + before;
    __builtin_amdgcn_wave_barrier();
    if (valid && before == 0) bin[l] = pos + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
    if (valid) {                                                     // pos < m: the bins were counted from the same lengths
      rank_out[i] = pos;
      sorted[pos] = id;
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += 128) {
    const int rt = pc[i], rc = pt[i];
    pc[i] = sorted_c[rt];
    pt[i] = sorted_t[rc];
  }
}
}  // namespace

extern "C" int nnr_cne_pair_triples(const int* beh_history, const int* cand, const int* tlen, const int* clen, long n, int H, int n_news,
                                    int batch_size, long first, long count, int* pc_hist, int* pt_hist, int* pc_cand, int* pt_cand, int* tmp,
                                    hipStream_t stream) {
  if (!beh_history || !cand || !tlen || !clen || !pc_hist || !pt_hist || !pc_cand || !pt_cand || !tmp) return NNR_ERR_ARG;
  if (H < 1 || n_news < 1 || batch_size < 1 || count < 1 || first < 0 || first % batch_size != 0 || first + count > n ||
      (first + count < n && count % batch_size != 0))
    return NNR_ERR_ARG;
  const long batches = (count + batch_size - 1) / batch_size;
  if ((long)batch_size * H > 0x7fffffffL || 2 * batches > 0x7fffffffL) return NNR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cne_pair_triples_kernel, dim3((unsigned)(2 * batches)), dim3(128), 0, stream, beh_history, cand, tlen, clen, H, n_news,
                     batch_size, first, count, pc_hist, pt_hist, pc_cand, pt_cand, tmp);
  NNR_CHECK_LAUNCH();
  return NNR_OK;
}
