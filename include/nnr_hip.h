/* libnnr_hip.so -- C-ABI of the MI355X-native NNR training hot path (gfx950 only).
 *
 * The reference (Veason-silverbullet/NNR) is pure Python; the native work on its hot path happens inside
 * third-party libraries that its modules call: ATen/cuDNN behind nn.LSTM / nn.Embedding / nn.Linear / bmm /
 * softmax, torch_scatter 2.0.9, and NCCL.  Each entry point below replaces
 * one such call site; the citation is the reference file:line whose arithmetic it implements.
 *
 * Conventions: extern "C"; plain pointers and sizes; every buffer is a caller-allocated
 * DEVICE pointer (the host side uses PyTorch's caching allocator purely as a memory manager); row-major,
 * contiguous unless a leading dimension is passed; kernels are enqueued on the caller's stream and never
 * synchronise with the host (token counts that depend on the data stay in device memory); returns NNR_OK or a
 * negative error code, never throws.  fp32 everywhere (the parity bar is 1e-4 fp32 on logits/loss).
 */
#ifndef NNR_HIP_H
#define NNR_HIP_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNR_OK 0
#define NNR_ERR_ARG (-1)
#define NNR_ERR_LAUNCH (-2)
#define NNR_ERR_UNSUPPORTED (-3)

int nnr_version(void);

/* ------------------------------------------------------------------------------------------------ GEMM
 * C[M,N] = epilogue(alpha * A_op[M,K] . B_op[K,N]).  Replaces every nn.Linear / torch.bmm on the path
 * (newsEncoders.py:122-123 input projection inside nn.LSTM, :128-129 title_H/title_M; layers.py:168 affine1,
 * :197 K/Q, :286 bmm(graph, x) and W; userEncoders.py:85-91) and their autograd backward GEMMs.
 *   trans_a = 0: A is [M,K], K contiguous (lda).        trans_a = 1: A is [K,M], M contiguous.
 *   trans_b = 0: B is [N,K], K contiguous (nn.Linear weight layout).   trans_b = 1: B is [K,N], N contiguous.
 *   Supported pairs: (0,0) forward, (0,1) data-gradient, (1,1) weight-gradient.
 * Epilogue order per element: x = alpha*acc; += bias[n]; += rowvec[map[m]][n]; act; aux_out = x; *= mul[m][n];
 * += resid[m][n]; dropout (drop_target 3); rowdot += rowdot_w[n]*x; store / accumulate / atomicAdd to C row c_idx[m].
 */
typedef struct nnr_gemm_args {
  const float* A;
  const float* B;
  float* C;                 /* may be NULL when only rowdot_out / aux_out are wanted */
  int M, N, K;
  int lda, ldb, ldc;
  int trans_a, trans_b;
  const int* dyn_dev;       /* device int32: actual extent of the token dimension (<= the static one) */
  int dyn_dim;              /* 0 none, 1: bounds M, 2: bounds K */
  const int* a_idx;         /* trans_a=0: A row m is read from A[a_idx[m]] (negative: zero row); embedding gather */
  const int* b_idx;         /* trans_b=1: B k-row is read from B[b_idx[k]] (negative: zero row) */
  int drop_target;          /* 0 none; 1 gathered-A element (m,k); 2 gathered-B element (k,n); 3 C element (m,n);
                               4 scattered atomic C element (m,n).  Element id = row * drop_cols + col. */
  float drop_p;
  uint32_t drop_seed;
  int drop_cols;
  float alpha;
  const float* bias;        /* [N] */
  const float* rowvec;      /* [*, ldrv] */
  int ldrv;
  const int* rowvec_map;    /* [M] or NULL */
  int act;                  /* 0 none, 1 relu, 2 tanh, 3 sigmoid */
  float* aux_out;           /* [M, ldaux]: value right after the activation */
  int ldaux;
  const float* mul;         /* [M, ldmul] */
  int ldmul;
  const float* resid;       /* [M, ldres] */
  int ldres;
  int accumulate;           /* 1: C += result (after the epilogue); 2: add the old C BEFORE bias/activation (k-split convs) */
  int atomic;               /* atomicAdd into C (implied by split_k > 1) */
  const int* c_idx;         /* [M]: destination row of C for row m (negative: skip) */
  int split_k;              /* > 1: reduction split over blockIdx.z, atomicAdd into a pre-zeroed C */
  const float* rowdot_w;    /* [N]; needs N <= 208 */
  float* rowdot_out;        /* [M] */
  int batch;                /* > 1: blockIdx.z batches with the strides below */
  long strideA, strideB, strideC, stride_aux, stride_res;
  int k_chunk;              /* > 0: like split_k but with fixed-size slices of k_chunk reduction rows (multiple of 32): the number of
                               live slices follows the device-side K; atomicAdd into a pre-zeroed / running C */
  float* colsum_out;        /* trans_a only: colsum_out[m] += sum_k A[k][m]  (fused bias gradient, f32 atomics) */
  int tile;                 /* 0: the library chooses (csrc/gemm.hip: choose_tile); else a row of csrc/gemm.hip's tile table kTiles, which states
                             * each id's kernel, shape and what it accepts (nnr_gemm_tile_info lists the rows): 2 3 4 5 6 register-staged,
                             * 7 skinny, 9 15 16 LDS-DMA NT, 20 26 27 30 32 LDS-DMA TN, 50 51 bf16x3 NT.  NNR_ERR_ARG when the row refuses the launch */
  /* filled by the library */
  uint32_t drop_thresh;
  float drop_scale;
  int vec_epi;
  /* reproducible split-K (trans_a = trans_b = 1, split_k > 1, N % 4 == 0): with `slab` set, slice z STORES its partial M x N result to
   * slab[z] and a second launch adds the live slices in slice order into C (and the fused column sums into colsum_out): no f32
   * atomics inside the reduction, bit-identical gradients from run to run (config.py:125-130).  slab_floats >= split_k * (M * N + M). */
  float* slab;
  long slab_floats;
  int slab_mode;            /* filled by the library */
  /* fused cross-selective gate backward (newsEncoders.py:128-131: Ht = H * G, G = sigmoid(pre)) in the epilogue of the GEMM that
   * completes dHt:  x = alpha * acc + pre_add[m][n];  aux_out[m][n] = x * resid * mul * (1 - mul)  (= d pre, resid = H, mul = G);
   * C[m][n] = x * mul  (= dH).  Needs the float4 epilogue (aligned operands, N % 4 == 0), no bias / activation / dropout. */
  const float* pre_add;     /* [M, ldpre]: added to the product before anything else (also without gate_bwd) */
  int ldpre;
  int gate_bwd;
  /* tile = 50 computes the same NT product on the BF16 matrix pipe as six exact bf16 x bf16 products with fp32 accumulation (an fp32 value is
   * exactly the sum of three bf16 values; error vs fp64 a third of the fp32-MFMA kernels'; round 5: measured, round 6: the host's default for
   * NT launches whose B is a weight).  Non-finite operands give non-finite outputs (+-Inf or NaN, not necessarily fp32's choice of the two); finite values up to FLT_MAX are
   * exact (csrc/gemm.hip: split3_bf16, split3_trunc8).  B3: the weight matrix B [N, K] pre-split by nnr_split_bf16x3 into three bf16 images [N, ldb3] (ldb3 % 8 == 0, zero-padded), image i at
   * B3 + i * b3_stride elements. */
  const void* B3;
  long b3_stride;
  int ldb3;
} nnr_gemm_args;

int nnr_gemm_f32(const nnr_gemm_args* args, hipStream_t stream);
/* Host-only: the tile id nnr_gemm_f32 would launch for these arguments (0: an empty product, nothing runs), or the negative code with which it
 * would refuse them.  Dereferences none of the data pointers. */
int nnr_gemm_tile_for(const nnr_gemm_args* args);
/* Host-only: row `index` (0, 1, ... until NNR_ERR_ARG) of the tile table for one operand layout.  dims[6] = id, rows, cols, reduction depth of a
 * stage, stage buffers, workgroups per CU the kernel is built for (0: no launch bound); suffix: the live profile's family is
 * gemm_<nt | nn | tn>_<suffix>; kernel: the instantiation as rocprofv3 prints it ("" for the skinny tile, which picks its wave count per launch).
 * cap >= 64 bytes each.  NNR_ERR_UNSUPPORTED: the row has no kernel for this layout. */
int nnr_gemm_tile_info(int index, int trans_a, int trans_b, int* dims, char* suffix, char* kernel, int cap);
/* w [rows, cols] (row stride ld) -> three bf16 images out3[i * img_stride + r * ldo + c] with w == image0 + image1 + image2 EXACTLY (columns
 * cols .. ldo-1 zero).  For nnr_gemm_args.B3 (experimental tile 50); weights change once per optimizer step. */
int nnr_split_bf16x3(const float* w, int rows, int cols, int ld, int ldo, void* out3, long img_stride, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ sequence planner
 * Replaces newsEncoders.py:106-120 (mask[:,0]=1 in place, lengths, torch.sort x2, index_select, pack_padded_sequence and
 * its sorted_length.cpu() host sync).  perm_in (optional, [n]): sorted position -> original row, when the caller wants a
 * specific tie order (e.g. the installed torch's unstable CPU sort); NULL = stable descending order computed on device.
 * Outputs: len_out[n], order[n], rank[n], slen[n], bs[L], off[L+1] (off[L] = #valid tokens, used as dyn_dev by the GEMMs),
 * row_seq[n*L], tok[n*L] (token id per packed row; NULL to skip), prev_f[n*L], prev_r[n*L]. */
int nnr_seq_plan(uint8_t* mask, const int* ids, int n, int L, const int* perm_in, int* len_out, int* order, int* rank, int* slen,
                 int* bs, int* off, int* row_seq, int* tok, int* prev_f, int* prev_r, hipStream_t stream);

/* The candidate call and the history call of one training step (model.py:123-125: the same news encoder applied to
 * [B, 1+neg] and to [B, max_history] news) planned as ONE packed token stream of n0 + n1 sequences, so that every per-token
 * kernel of the step runs once over both calls.  Rows [0, n0) of every per-sequence array come from mask0 / ids0, rows
 * [n0, n0+n1) from mask1 / ids1; both masks get the mask[:,0]=1 fix in place.  Other arguments as nnr_seq_plan. */
int nnr_seq_plan_pair(uint8_t* mask0, const int* ids0, int n0, uint8_t* mask1, const int* ids1, int n1, int L, const int* perm_in,
                      int* len_out, int* order, int* rank, int* slen, int* bs, int* off, int* row_seq, int* tok, int* prev_f,
                      int* prev_r, hipStream_t stream);

/* CNE's rank pairing (newsEncoders.py:112-115,128-129: the title sequence at sorted position r of a call is gated by the cell
 * state of the CONTENT sequence at sorted position r of the same call, and vice versa) for two calls planned as one union
 * stream: order_t / order_c = nnr_seq_plan_pair's `order` of the title / content stream; pm_t[s] = position in the content
 * stream's union order of the partner of the title sequence at position s, pm_c[s] the reverse (pm_c = pm_t^-1).
 * tmp: 4 * n ints of scratch. */
int nnr_cne_pair_map(const int* order_t, const int* order_c, int n0, int n, int* pm_t, int* pm_c, int* tmp, hipStream_t stream);

/* Packed token rows for the MHSA news encoder (round 5).  cover[i][t] = 1 for t <= the last valid position of title i (all ones for a title
 * with no valid position: its softmax over -1e9 scores is uniform, every position counts -- newsEncoders.py:187-200, layers.py:142-143,171);
 * nnr_seq_plan on `cover` packs exactly the rows that can reach the result, and rowmap[i*L + t] = off[t] + rank[i] (t < len[i], else -1)
 * tells nnr_mhsa_fwd_packed / nnr_mhsa_bwd_packed where position t of title i lives. */
int nnr_mask_cover(const uint8_t* mask, int n, int L, uint8_t* cover, hipStream_t stream);
int nnr_seq_rowmap(const int* off, const int* rank, const int* len, int n, int L, int* rowmap, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ Bi-LSTM
 * Replaces nn.LSTM(bidirectional) on a PackedSequence (newsEncoders.py:66-67, 119-127) and its backward.
 * Gate columns are kept in "p-order": p = (unit/16)*64 + (unit%16)*4 + gate, padded to NP = ceil(H/16)*64 per direction. */
int nnr_lstm_dims(int H, int* UB, int* HP, int* NP);
/* w_ihp [2*NP, E], b_p [2*NP] (= b_ih + b_hh), wf [2*UB*4*UB*256], wb [2*UB*(NP/16)*256]; w_ihp_t (optional) [E, 2*NP] = w_ihp^T,
 * the K-contiguous operand of the embedding-row gradient GEMM */
int nnr_lstm_pack_weights(const float* w_ih_f, const float* w_hh_f, const float* b_ih_f, const float* b_hh_f, const float* w_ih_r,
                          const float* w_hh_r, const float* b_ih_r, const float* b_hh_r, int H, int E, float* w_ihp, float* b_p,
                          float* wf, float* wb, float* w_ihp_t, hipStream_t stream);
/* dw_ihp [2*NP, E], db_p [2*NP], dw_hhp [2, NP, H] -> gradients in nn.LSTM's parameter layout.  zero_src != 0: the packed buffers are
 * returned all-zero (a persistent workspace the next step's split-K GEMMs accumulate into again: no per-step fill launches). */
int nnr_lstm_unpack_grads(float* dw_ihp, float* db_p, float* dw_hhp, int H, int E, float* dw_ih_f, float* dw_hh_f,
                          float* db_ih_f, float* db_hh_f, float* dw_ih_r, float* dw_hh_r, float* db_ih_r, float* db_hh_r,
                          int accumulate /* 0: overwrite, 1: atomic += */, int zero_src, hipStream_t stream);
typedef struct nnr_lstm_problem {
  const int* bs; const int* off; const int* slen; const int* prev_f; const int* prev_r;   /* from nnr_seq_plan */
  int n, L;
  float* gates;       /* [rows, 2*NP]  fwd: in = x.W_ihp^T + b_p, out = activated gates; bwd: in = gates, out = d(pre-activations) */
  float* cell;        /* [rows, 2*HP]  c_t */
  float* hout;        /* [rows, 2*H]   h_t = [fwd | rev] */
  float* cn;          /* [n, 2*H]      final cell states in sorted order */
  const float* wf;    /* forward fragment-layout W_hh */
  const float* wb;    /* backward fragment-layout W_hh */
  const float* dh;    /* bwd: dL/dH [rows, 2*H] */
  const float* dcn;   /* bwd: dL/dc_n [n, 2*H] or NULL */
  unsigned* sync;     /* optional workspace of nnr_lstm_sync_bytes(n) bytes, ZERO-FILLED ONCE BY THE CALLER before its first launch
                       * and reusable by later launches without clearing (exchange words carry a per-launch epoch; one workspace
                       * must not be shared by two launches that can be in flight together): when every problem of a
                       * launch has one and H is even with 13 unit blocks (194 <= H <= 208; the product's H = 200), each
                       * 16-sequence tile runs on a PAIR of CUs with W_hh resident in registers/LDS, exchanging half of
                       * h_t per step (every other H, odd ones included, runs the one-CU kernels and leaves the
                       * workspace alone); after the launch the 64 bytes at
                       * nnr_lstm_sync_diag_offset(n) hold diagnostics (word 0 = spin-wait time-outs of that launch, must be 0) */
} nnr_lstm_problem;
size_t nnr_lstm_sync_bytes(int n);
size_t nnr_lstm_sync_diag_offset(int n);   /* byte offset of the diagnostics block inside that workspace */
/* Registers a caller-owned, zero-initialised device counter that every exchange time-out of every later launch adds to (NULL
 * unregisters).  A time-out is a data-poisoning event, not a retry: the waiting lane continues with NaN, the step's loss and
 * gradient norm become NaN, and nnr_clip_adam leaves parameters and moments untouched for such a step.  (The reference has no
 * counterpart: cuDNN's nn.LSTM is one kernel, newsEncoders.py:119-127.) */
int nnr_lstm_set_timeout_counter(unsigned* dev_counter);
/* up to 4 problems (title + content streams of the candidate call and of the history call) run in ONE launch: the
 * recurrence is bound by its longest dependent chain, so independent streams are free to share it */
int nnr_lstm_fwd(const nnr_lstm_problem* probs, int nprob, int H, hipStream_t stream);
int nnr_lstm_bwd(const nnr_lstm_problem* probs, int nprob, int H, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ GRU
 * Replaces nn.GRU on a PackedSequence (userEncoders.py:287-332) and its backward, csrc/gru.hip.  Every unit has four slots
 * [r, z, n_x, n_h] in p-order: p = (unit/16)*64 + (unit%16)*4 + slot, padded to NP = ceil(H/16)*64.
 * Supported: 1 <= H <= 256 and 1 <= T <= 255, anything else is NNR_ERR_UNSUPPORTED. */
int nnr_gru_dims(int H, int T, int* UB, int* HP, int* NP);
/* w_ih [3H, D], w_hh [3H, H], b_ih [3H], b_hh [3H] (gate order r | z | n) -> w_ihp [NP, D] (slot 3 rows zero),
 * b_p [NP] = (b_ir + b_hr, b_iz + b_hz, b_in, b_hn), wf [UB*3*UB*256] (forward fragments), wb [UB*(NP/16)*256] (backward fragments) */
int nnr_gru_pack_weights(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int H, int D, float* w_ihp,
                         float* b_p, float* wf, float* wb, hipStream_t stream);
/* dw_ihp [NP, D], db_p [NP], dw_hhp [NP, H] (products / column sums over the buffer nnr_gru_bwd leaves) are ADDED to the gradients in
 * nn.GRU's parameter layout, one writer per element (no atomics) */
int nnr_gru_unpack_grads(const float* dw_ihp, const float* db_p, const float* dw_hhp, int H, int D, float* dw_ih, float* dw_hh,
                         float* db_ih, float* db_hh, hipStream_t stream);
/* gates [B*T, NP]: in = x . w_ihp^T + b_p for every history slot, out = (r, z, n, W_hn h + b_hn) at the live ones.  mask uint8 [B, T]:
 * len[b] = number of non-zero entries (written to len [B]); user b runs slots 0 .. len[b]-1 and keeps h afterwards.  h0 [B, H] or NULL
 * (zeros).  hout / hprev [B*T, H]: h_t / h_{t-1} at the live slots (the rest is left untouched), hfinal [B, H]. */
int nnr_gru_fwd(float* gates, const unsigned char* mask, const float* h0, const float* wf, int B, int T, int H, float* hout,
                float* hprev, float* hfinal, int* len, hipStream_t stream);
/* gates: in = what nnr_gru_fwd left, out = d(pre-activations) (dr, dz, dn, dn r), ZERO at every dead slot; dhfinal [B, H];
 * dh0 [B, H] or NULL receives dL/dh0 (= dhfinal for a user without history) */
int nnr_gru_bwd(float* gates, const int* len, const float* hprev, const float* wb, const float* dhfinal, int B, int T, int H,
                float* dh0, hipStream_t stream);
/* the decoder's tail: rows of users without history are exactly zero (not tanh(bias)); dz = dy (1 - y^2), zero for those rows */
int nnr_gru_zero_empty(float* y, const int* len, int B, int D, hipStream_t stream);
int nnr_gru_tanh_bwd(const float* dy, const float* y, const int* len, int B, int D, float* dz, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ attention pooling
 * softmax(mask(score)) . x : the tails of `Attention` (layers.py:169-175) and `ScaledDotProduct_CandidateAttention`
 * (layers.py:197-203), forward and backward; see pool.hip for the layouts.  D <= 1280, L <= 128; D, ldx, ldth and the leading
 * dimension of every operand whose pointer is set are multiples of 4 (rows move as float4), else NNR_ERR_UNSUPPORTED. */
typedef struct nnr_pool_args {
  const float* x; int ldx; int D; int n; int L;
  int packed;                                /* 1: time-major packed rows (off/slen/order), 0: dense [n, L, D] */
  const int* off; const int* slen; const int* order;
  const uint8_t* mask; int mask_div;         /* dense only: mask[(s / mask_div) * L + t] */
  const float* score;                        /* given scores (per row) ... */
  const float* v; int ldv; float scale;      /* ... or score = scale * <x, v[out index]> */
  float* alpha;
  float* out; int ldo; const float* add_in; int ldadd;     /* out = pooled (+ add_in) */
  const float* dout; int lddo; const float* dout2; int lddo2;   /* backward: upstream = dout (+ dout2) */
  float* dx; int lddx; int dx_accumulate;
  float* dscore;
  float* dv; int lddv;
  /* forward only, instead of `score`: score[row] = <th[row, :A], w2>  (the w2 . tanh(.) of layers.py:168 computed in the pool's
   * own pass over the tokens; A <= 256, A % 4 == 0, th rows laid out like x) */
  const float* th; int ldth; int A; const float* w2;
  /* backward only (round 5): the token gradient of a SECOND pool over the same x, folded into this call's ONE write of dx:
   *   dx[row] = alpha[row] * (dout + dout2)  +  alpha_b[row] * dout_b[out index]  +  scale_b * dscore_b[row] * v_b[out index]
   * CNE pools every token stream twice (self attention, layers.py:167-175, and cross attention, layers.py:196-203, newsEncoders.py:
   * 132-137): the cross pool's backward (which must run first: its dv feeds the OTHER stream's self vector) is called with dx = NULL
   * and only writes dscore / dv; the self pool's backward then writes dH~ once instead of write + read-modify-write.  All NULL / 0: off. */
  const float* alpha_b; const float* dout_b; int lddo_b; const float* dscore_b; const float* v_b; int ldv_b; float scale_b;
} nnr_pool_args;
int nnr_attn_pool_fwd(const nnr_pool_args* a, hipStream_t stream);
int nnr_attn_pool_bwd(const nnr_pool_args* a, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ elementwise / reductions */
int nnr_gate_bwd(const float* dHt, const float* H, const float* G, float* dH, float* dpre, const int* rows_dev, int rows, int cols,
                 hipStream_t stream);                                            /* newsEncoders.py:128-131 backward */
int nnr_packed_seq_sum(const float* x, int D, const int* off, const int* slen, int n, float* out, hipStream_t stream);
/* `ws`: NULL (f32 atomics straight into the destination: arrival order, not reproducible), or a workspace of
 * nnr_slot_workspace_floats(N) floats owned by the calling stream: every workgroup stores the column sums of its share of the live
 * rows to its own slot row, and a second tiny launch adds the slot rows in a fixed order into the destination (one f32 atomic per
 * column and call) -- bit-identical from run to run, and no serialisation on the destination's few cache lines. */
int nnr_slot_workspace_floats(int N);
int nnr_tanh_score_bwd(float* th, const float* ds, const float* w2, float* dw2, const int* rows_dev, int rows, int A, float* ws,
                       hipStream_t stream);                                      /* layers.py:168-169 backward */
int nnr_colsum(const float* x, int ld, const int* rows_dev, int rows, int N, float* out_accum, float* ws, hipStream_t stream);
int nnr_rowdot(const float* x, int ld, const float* w, const int* rows_dev, int rows, int N, float* out,
               hipStream_t stream);                                              /* out[row] = <x[row, :N], w>  (layers.py:168) */
int nnr_small_embed_fwd(const float* table, const int* idx, int n, int dim, float* out, int ldo, float p, uint32_t seed,
                        hipStream_t stream);                                     /* newsEncoders.py:51-53 */
int nnr_small_embed_bwd(const int* idx, int n, int dim, const float* dout, int lddo, float* dtable_accum, float p, uint32_t seed,
                        hipStream_t stream);
/* The user-id embedding table of the personalised encoders (model.py:122-125): out[b,:] = dropout(table[ids[b],:]), mask keyed by the
 * output element b*dim + c; dtable[u,:] += sum over b with ids[b] == u, in ascending b, of mask * dout[b,:] (one writer per row: no float
 * atomics, same inputs same bits).  table / dtable [rows, dim], ids int64 [B].  An id outside [0, rows) yields a zero row and contributes no
 * gradient; nothing outside the rows x dim table is read or written. */
int nnr_user_rows_fwd(const float* table, int rows, const int64_t* ids, int B, int dim, float* out, float p, uint32_t seed,
                      hipStream_t stream);
int nnr_user_rows_bwd(const float* dout, const int64_t* ids, int B, int rows, int dim, float* dtable_accum, float p, uint32_t seed,
                      hipStream_t stream);
/* nn.Embedding forward / backward for a dense id tensor (newsEncoders.py:117-118, 163, 193) with the in-place dropout fused:
 * out[row,:] = dropout(table[idx[row],:]) (negative idx: zero row); dtable[idx[row],:] += mask * dout[row,:] (f32 atomics). */
int nnr_embed_gather(const float* table, const int* idx, long n, const int* n_dev /* optional live row count */, int dim, float* out,
                     float p, uint32_t seed, hipStream_t stream);
int nnr_embed_scatter(const float* dout, const int* idx, long n, int dim, float* dtable_accum, float p, uint32_t seed,
                      hipStream_t stream);
/* the same over the first min(n, *n_dev) rows (packed token streams: the live row count stays on the device) */
int nnr_embed_scatter_dyn(const float* dout, const int* idx, long n, const int* n_dev, int dim, float* dtable, float p, uint32_t seed,
                          hipStream_t stream);
/* Reproducible form of the embedding-row gradient (the reference's runs are seeded and deterministic: config.py:125-130; autograd's
 * nn.Embedding backward at newsEncoders.py:117-118).  nnr_token_sort: stable sort of the live packed rows by word id (rows beyond
 * min(cap, *n_dev) and ids outside [0, vocab) get the pad key `vocab` and sort to the end); keys_tmp / rows_tmp / keys_sorted /
 * rows_sorted: `cap` entries each, temp: nnr_token_sort_workspace_bytes(cap, vocab) bytes.  It needs nothing but the planned token
 * stream, so the host side issues it on a side stream under the forward pass.  nnr_embed_scatter_sorted: dtable[w,:] += sum of
 * mask * dout[row,:] over the rows of word w IN LIST ORDER -- every word receives ONE f32 atomic add per element and launch, so
 * with at most two launches per step into a zeroed table gradient (title stream, content stream) the result is bit-reproducible;
 * partial_ws: nnr_embed_scatter_sorted_workspace_floats(cap) floats; dim <= 320. */
size_t nnr_token_sort_workspace_bytes(long cap, int vocab);
int nnr_token_sort(const int* tok, long cap, const int* n_dev, int vocab, unsigned* keys_tmp, int* rows_tmp, unsigned* keys_sorted,
                   int* rows_sorted, void* temp, size_t temp_bytes, hipStream_t stream);
size_t nnr_embed_scatter_sorted_workspace_floats(long cap);
int nnr_embed_scatter_sorted(const float* dout, const unsigned* keys_sorted, const int* rows_sorted, long cap, int vocab, int dim,
                             float* dtable_accum, float p, uint32_t seed, float* partial_ws, hipStream_t stream);
int nnr_transpose2d(const float* in, float* out, long rows, int cols, int accumulate, hipStream_t stream);
/* `count` independent transposes out[c][r] = in[r][c] in ONE launch; the descriptors live in device memory (the host side keeps
 * them for the W^T copies of the weights that the data-gradient GEMMs multiply by: refreshed once per optimizer step). */
typedef struct nnr_transpose_desc { const float* in; float* out; int rows, cols; } nnr_transpose_desc;
int nnr_transpose_batch(const nnr_transpose_desc* descs_dev, int count, hipStream_t stream);
/* Strided permute of at most four axes: out[i0 so0 + i1 so1 + i2 so2 + i3 so3] (+)= in[i0 si0 + i1 si1 + i2 si2 + i3 si3] for 0 <= id < nd
 * (accumulate != 0: added to what is there, one plain writer per element).  Strides are in floats; unused leading axes have extent 1.
 * Source strides may be negative: the caller passes `in` offset so that every address lies inside the source.  Threads walk the index
 * space row-major, i3 fastest, so the caller makes i3 the destination's unit-stride axis (coalesced writes, strided reads).  Elements of
 * `out` that no index reaches are not touched.  This is how every weight takes the layout its product reads, once per parameter version
 * (KCNN, HDC, FIM below).  NNR_ERR_ARG: a null pointer or an extent < 1; NNR_ERR_UNSUPPORTED: n0 n1 n2 n3 >= 2^31. */
int nnr_permute(const float* in, float* out, int n0, int n1, int n2, int n3, long si0, long si1, long si2, long si3, long so0, long so1,
                long so2, long so3, int accumulate, hipStream_t stream);
int nnr_add(float* y, const float* x, long n, float alpha, hipStream_t stream);
int nnr_add_atomic(float* y, const float* x, long n, float alpha, hipStream_t stream);   /* y += alpha*x with f32 atomics */
int nnr_add2d(float* y, int ldy, const float* x, int ldx, int rows, int cols, float alpha, int accumulate, hipStream_t stream);
/* y[b, j, :] = x[b, :] for j < N -- the user vector repeated over the candidates (userEncoders.py:172 `.repeat`, :190 `.expand`) -- and its
 * backward dx[b, :] = sum_j dy[b, j, :] (ascending j).  x / dx [B, D], y / dy [B, N, D], contiguous. */
int nnr_expand_rows_fwd(const float* x, float* y, int B, int N, int D, hipStream_t stream);
int nnr_expand_rows_bwd(const float* dy, float* dx, int B, int N, int D, hipStream_t stream);
int nnr_dropout(const float* x, float* y, long n, float p, uint32_t seed, hipStream_t stream);
int nnr_relu_bwd(const float* dy, const float* y, float* dx, long n, hipStream_t stream);
/* SUE's per-user graph aggregate (layers.py:285-292: `graph @ feature` inside GCNLayer.forward, B users x [G, G] x [G, D]) with
 * GCNLayer's epilogue:  y = dropout(relu?(graph_b . z_b + bias) + resid), r_out (optional) = the value after bias / ReLU (what the
 * backward mask needs).  G <= 128.  p / seed: counter-based dropout over the flat [B, G, D] index (same mask as nnr_relu_drop_bwd). */
int nnr_gcn_aggregate_fwd(const float* graph, const float* z, const float* bias, const float* resid, float* r_out, float* y, int B, int G,
                          int D, int relu, float p, uint32_t seed, hipStream_t stream);
/* Its backward:  ds = mask(dy) * (r > 0), dx0 (optional) = mask(dy) (the residual branch), dz_b = graph_b^T . ds_b.  r == NULL: plain
 * dz_b = graph_b^T . dy_b (ds / dx0 untouched). */
int nnr_gcn_aggregate_bwd(const float* graph, const float* dy, const float* r, float* ds, float* dx0, float* dz, int B, int G, int D, float p,
                          uint32_t seed, hipStream_t stream);
int nnr_relu_drop_bwd(const float* dy, const float* r, float* ds, float* dx, long n, float p, uint32_t seed, hipStream_t stream);
/* Backward of y = dropout(sigmoid(z)) given s = sigmoid(z) (the dense layers of the DAE news encoder, newsEncoders.py:389-390):
 * dz = mask(dy) * s * (1 - s); same mask as nnr_relu_drop_bwd. */
int nnr_sigmoid_drop_bwd(const float* dy, const float* s, float* dz, long n, float p, uint32_t seed, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ multi-head self-attention core
 * MultiHeadAttention.forward after the W_Q/W_K/W_V projections (layers.py:137-147) on v_mfma_f32_32x32x2_f32:
 * qkv [n*Lq, 3*heads*dh] = [Q | K | V] (head h at columns h*dh), key mask [n, Lq] (0 -> -1e9) or NULL, scale = 1/sqrt(dh);
 * out [n*Lq, heads*dh]; prob [n*heads, NB*NB*1024] (NB = 1 for Lq <= 32, 2 for Lq <= 64) saved for backward, or NULL in
 * both calls: backward then recomputes the probabilities from Q, K (the product path does this).
 * drop_p > 0 fuses the dropout that follows the attention (newsEncoders.py:196): out = nnr_dropout(O, drop_p, seed) bit for bit
 * (mask = f(seed, flat index in out)), and backward applies the same mask to dout while staging it. */
int nnr_mhsa_fwd(const float* qkv, const uint8_t* mask, int n, int Lq, int heads, int dh, float scale, float* out, float* prob,
                 float drop_p, uint32_t seed, hipStream_t stream);
int nnr_mhsa_bwd(const float* qkv, const uint8_t* mask, const float* prob, const float* dout, int n, int Lq, int heads, int dh,
                 float scale, float* dqkv, float drop_p, uint32_t seed, hipStream_t stream);
/* The same over PACKED token rows: qkv / out / dout / dqkv hold only the rows rowmap names (position t of sample i at row rowmap[i*Lq + t],
 * -1 = no such row: reads as zero, is not stored); `mask` is still the dense [n, Lq] key mask.  Needs heads % 4 == 0, dh % 4 == 0, Lq <= 32
 * rows per 4-head group as in the dense cooperative path; dropout indices are (packed row) * heads*dh + column. */
int nnr_mhsa_fwd_packed(const float* qkv, const uint8_t* mask, const int* rowmap, int n, int Lq, int heads, int dh, float scale, float* out,
                        float drop_p, uint32_t seed, hipStream_t stream);
int nnr_mhsa_bwd_packed(const float* qkv, const uint8_t* mask, const int* rowmap, const float* dout, int n, int Lq, int heads, int dh, float scale,
                        float* dqkv, float drop_p, uint32_t seed, hipStream_t stream);
/* Round 6: PAIRED short titles.  The attention core multiplies 32 x 32 blocks whatever a title's length, and 85 % of MIND-shaped titles cover <= 16
 * positions; nnr_mhsa_pair_map lays the titles of a packed call (Lq = 32) out as virtual samples in the plan's sorted order -- the titles covering
 * more than 16 positions alone, the others two to a sample (positions 0..15 / 16..31) -- and nnr_mhsa_fwd_paired / _bwd_paired run the core over
 * them, with -inf scores between the two titles of a pair (exact zeros in every product that follows).  Same results as nnr_mhsa_*_packed up to
 * the order of fp32 additions inside a softmax row; ~0.6x of its matrix work.  vrowmap / vmask: [n, 32]; off: the plan's offsets (off[17] - off[16]
 * = the number of unpaired titles).  layers.py:132-148. */
int nnr_mhsa_pair_map(const int* off, const int* slen, const int* order, const uint8_t* mask, int n, int L, int* vrowmap, uint8_t* vmask,
                      hipStream_t stream);
int nnr_mhsa_fwd_paired(const float* qkv, const uint8_t* vmask, const int* vrowmap, const int* off, int n, int heads, int dh, float scale,
                        float* out, float drop_p, uint32_t seed, hipStream_t stream);
int nnr_mhsa_bwd_paired(const float* qkv, const uint8_t* vmask, const int* vrowmap, const int* off, const float* dout, int n, int heads, int dh,
                        float scale, float* dqkv, float drop_p, uint32_t seed, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ SUE (userEncoders.py:68-98) */
/* cmask_fix (optional): the [B, Kc + 1] cluster mask; its last column is set to 1 in place by the same launch (:73).
 * dx0_add (optional): second addend of the upstream gradient (the outer residual of :81), dX0 = dx0 + dx0_add. */
int nnr_sue_x0_fwd(const float* hist, const float* proxy, float* x0, int B, int Hn, int Kc, int D, float p, uint32_t seed,
                   uint8_t* cmask_fix, hipStream_t stream);                      /* :80 */
int nnr_sue_x0_bwd(const float* dx0, const float* dx0_add, float* dhist, float* dproxy_accum, int B, int Hn, int Kc, int D, float p,
                   uint32_t seed, hipStream_t stream);
int nnr_sue_slice_fwd(const float* gcn, const float* x0, float* gfeat, int B, int Hn, int G, int D, hipStream_t stream);   /* :81-82 */
int nnr_sue_slice_bwd(const float* dgfeat, float* dpad, int B, int Hn, int G, int D, hipStream_t stream);
/* torch_scatter.scatter_softmax + scatter_sum (userEncoders.py:85-89): kf [B,Hn,A], qc [B,N,A], g [B,Hn,D], cidx int64 [B,Hn]
 * (clamped into [0, C)) -> alpha [B,N,Hn], feat [B,N,C,D]; ds_ws [B*N*Hn] scratch.  Sizes as for the GEMV form below, and A >= 1: anything else is
 * NNR_ERR_UNSUPPORTED before any launch; a null pointer is NNR_ERR_ARG. */
int nnr_sue_intra_fwd(const float* kf, const float* qc, const float* g, const long* cidx, int B, int N, int Hn, int C, int A, int D,
                      float* alpha, float* feat, hipStream_t stream);
int nnr_sue_intra_bwd(const float* kf, const float* qc, const float* g, const long* cidx, const float* alpha, const float* dfeat, int B,
                      int N, int Hn, int C, int A, int D, float* dg, float* dkf, float* dqc, float* ds_ws /* [B*N*Hn] scratch */,
                      hipStream_t stream);
/* The same segmented pool in GEMV form (SUE_wo_GCN, variantEncoders.py:377-381; the key projection's bias cancels in every segment softmax,
 * so K(x_h) . q_n = x_h . u_n with u_n = W_K^T q_n):  x [B,Hn,D], u [B*N,D], cidx int64 [B,Hn] (clamped into [0, C)) -> alpha [B,N,Hn] =
 * softmax of scale <x_h, u_n> within each cluster, feat [B*N*C, D] = sum of alpha_h x_h over a cluster's members in ascending h (an empty
 * cluster's row is exactly 0).  Backward: dx [B,Hn,D] is written (not accumulated), du [B*N,D] = scale sum_h ds_h x_h; ds_ws [B*N*Hn] scratch.
 * No atomics: same inputs, same bits.  NNR_ERR_UNSUPPORTED, before any launch, unless 1 <= Hn <= 64, 1 <= C <= 32, 1 <= N <= 8, B >= 1, D >= 1. */
int nnr_sue_seg_pool_fwd(const float* x, const float* u, const long* cidx, int B, int N, int Hn, int C, int D, float scale, float* alpha,
                         float* feat, hipStream_t stream);
int nnr_sue_seg_pool_bwd(const float* x, const float* u, const long* cidx, const float* alpha, const float* dfeat, int B, int N, int Hn, int C,
                         int D, float scale, float* dx, float* du, float* ds_ws, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ candidate-aware additive attention
 * CATT (userEncoders.py:213-220, act = 1 relu) and layers.CandidateAttention / MultipleCandidateAttention (layers.py:225-232, 254-262,
 * act = 2 tanh), csrc/cand_attn.hip:  a[b,n,h] = w2 . act(P[b,n,:] + Q[b,h,:]);  alpha[b,n,:] = softmax_h(mask[b,h] ? a : -1e9);
 * out[b,n,:] = sum_h alpha[b,n,h] feat[b,h,:].   P [B*N, A] = query projection + bias, Q [B*H, A] = feature projection, w2 [A],
 * feat [B, H, D] with row stride ldf, mask uint8 [B, H] or NULL (no masking), alpha [B, N, H], out / dout [B, N, D]; all fp32.
 * The score's bias is no argument: it cancels in the softmax and its gradient is zero.
 * Backward: dP [B*N, A], dQ [B*H, A] and dfeat [B, H, D] are written (dfeat added into when dfeat_accumulate), dw2 [A] is ADDED into;
 * ws: nnr_cand_attn_ws_floats(B, N, H, A) floats of scratch owned by the calling stream.  Same inputs, same bits (no float atomics
 * into shared destinations but nnr_colsum's one add per column).  NNR_ERR_UNSUPPORTED when N*A + A + N*H floats exceed 64 KB of LDS. */
int nnr_cand_attn_ws_floats(int B, int N, int H, int A);
int nnr_cand_attn_fwd(const float* P, const float* Q, const float* w2, const float* feat, int ldf, const uint8_t* mask, int B, int N,
                      int H, int A, int D, int act, float* alpha, float* out, hipStream_t stream);
int nnr_cand_attn_bwd(const float* P, const float* Q, const float* w2, const float* feat, int ldf, const uint8_t* mask, const float* alpha,
                      const float* dout, int B, int N, int H, int A, int D, int act, float* dP, float* dQ, float* dfeat,
                      int dfeat_accumulate, float* ws, float* dw2_accum, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ per-title personalised attention
 * PNE's word-level attention (newsEncoders.py:359-360), csrc/pers_attn.hip: layers.CandidateAttention with the query taken through an
 * index map.  a[i,t] = w2 . tanh(Qf[i,t,:] + P[uidx[i],:]);  alpha[i,:] = softmax_t(mask[i,t] ? a : -1e9) (no live position: 1/L over all
 * L);  out[i,:] = sum_t alpha[i,t] feat[i,t,:].  Qf [n*L, A] = feature projection, P [U, A] = query projection + bias, uidx int32 [n]
 * (an entry outside [0, U): P = 0 for that title, and it joins no dP row), w2 [A], feat [n, L, F] with row stride ldf, mask uint8 [n, L]
 * or NULL, alpha [n, L], out / dout [n, F]; all fp32.  Backward: dP [U, A] (a user without titles: a zero row), dQf [n*L, A] (zero rows
 * where masked) and dfeat [n, L, F] are written, dw2 [A] is ADDED into; ws: nnr_pers_attn_ws_floats(n, L, A) floats of scratch owned by
 * the calling stream.  Same inputs, same bits.  NNR_ERR_UNSUPPORTED when L > 64 or A > 1024 (A > 256 on the scalar-lane path, taken
 * when A, F or ldf is no multiple of 4 or a base pointer is not 16-byte aligned). */
int nnr_pers_attn_ws_floats(int n, int L, int A);
int nnr_pers_attn_fwd(const float* Qf, const float* P, const int* uidx, int U, const float* w2, const float* feat, int ldf,
                      const uint8_t* mask, int n, int L, int A, int F, float* alpha, float* out, hipStream_t stream);
int nnr_pers_attn_bwd(const float* Qf, const float* P, const int* uidx, int U, const float* w2, const float* feat, int ldf,
                      const uint8_t* mask, const float* alpha, const float* dout, int n, int L, int A, int F, float* dP, float* dQf,
                      float* dfeat, float* ws, float* dw2_accum, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ OMAP (Hi-Fi Ark) user encoder
 * userEncoders.py:357-374, csrc/omap.hip.  hist [B, H, D] with row stride ldf (X), cand [B, N, D] (C), mask uint8 [B, H] or NULL (no
 * masking), W [D, K], s = sqrt(D):   alpha = softmax_j(mask[b,j] ? X X^T / s : -1e9) [B, H, H];  Y = X + alpha X [B, H, D];
 * beta = softmax_k(mask[b,i] ? Y W / s : -1e9) [B, H, K] (a padded row carries 1 / K and contributes to every archive);  R = beta^T Y
 * [B, K, D];  gamma = softmax_k(C R^T / s) [B, N, K];  out = gamma R [B, N, D].  A user without history has alpha = 1 / H.  All fp32; the
 * [H, H, D] products run on the exact-fp32 MFMA.  alpha, Y, beta, R and gamma are written by the forward call and read by the backward one.
 * Backward: dhist [B, H, D] contiguous (added into when dhist_accumulate) and dcand [B, N, D] are written, dW [D, K] is ADDED into; masked
 * scores pass no gradient (db = 0 on padded rows, dS = 0 on masked keys, also for a user without history).  ws: nnr_omap_ws_floats(B, N, H,
 * D, K) floats of scratch owned by the calling stream, for either call.  Same inputs, same bits: no float atomics.
 * NNR_ERR_UNSUPPORTED (from nnr_omap_ws_floats too, before any launch) when H > 96, K > 16 or (H + N) * K > 4096.
 * The regulariser coef * ||(W^T W) o (J_K - I_K)||_F: nnr_omap_reg_fwd writes the 0-dim loss and keeps Off [K * K] and Omega in off
 * [K * K + 1]; nnr_omap_reg_bwd ADDS gup[0] * coef * 2 W Off / Omega into dW (gup: device pointer to the upstream gradient; nothing is
 * added when Omega == 0, torch's subgradient).  Neither synchronises with the host. */
int nnr_omap_ws_floats(int B, int N, int H, int D, int K);
int nnr_omap_fwd(const float* hist, int ldf, const float* cand, const uint8_t* mask, const float* W, int B, int N, int H, int D, int K,
                 float* alpha, float* Y, float* beta, float* R, float* gamma, float* out, float* ws, hipStream_t stream);
int nnr_omap_bwd(const float* hist, int ldf, const float* cand, const uint8_t* mask, const float* W, const float* alpha, const float* Y,
                 const float* beta, const float* R, const float* gamma, const float* dout, int B, int N, int H, int D, int K, float* dhist,
                 int dhist_accumulate, float* dcand, float* dW_accum, float* ws, hipStream_t stream);
int nnr_omap_reg_fwd(const float* W, int D, int K, float coef, float* off, float* loss, hipStream_t stream);
int nnr_omap_reg_bwd(const float* W, const float* off, const float* gup, int D, int K, float coef, float* dW_accum, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ bag of words (csrc/bag.hip)
 * The masked mean of word-embedding rows that opens the DAE (newsEncoders.py:386-387) and Inception (newsEncoders.py:422-425) news
 * encoders, over the live positions of up to two token streams per news row: ids int32 [n, La] / [n, Lb], masks uint8 [n, La] / [n, Lb]
 * (ids_b == NULL with Lb == 0: one stream), table [V, E].  An id outside [0, V) counts as a live position with a zero row.
 *   separate == 0 (DAE):  out[r, off_a : off_a + E] = act((sum over both streams) / (count_a + count_b)); count [n].
 *   separate == 1 (Inception): the launch first sets mask[r, 0] = 1 IN PLACE on both streams; out[r, off_a : +E] = act(mean of stream a),
 *   out[r, off_b : +E] = act(mean of stream b); count [2, n] (stream a, then stream b).
 * act: 0 none, 3 sigmoid.  fp32 sums in a fixed order (stream a ascending, then stream b ascending), plain IEEE division: a row with no
 * live position gives 0 / 0.  tok (optional) int32 [n, La + Lb] receives the word id of every live position and -1 elsewhere: sorted by
 * nnr_token_sort (cap = n * (La + Lb), n_dev = NULL) it is the occurrence list the backward call reads.
 * Backward: dtable[w, :] += sum over the live occurrences (r, pos) of w, in sorted-list order, of g[r] / count, with g[r] = dout[r, off :
 * off + E] for act 0 and dout * out * (1 - out) for act 3 (out: the forward call's output; may be NULL for act 0).  No [tokens, E]
 * buffer is read or written; no float atomics: every table row has one writer, so concurrent calls must not share dtable rows.
 * partial_ws: nnr_bag_mean_bwd_ws_floats(cap) floats.  Same inputs, same bits.
 * NNR_ERR_UNSUPPORTED when La > 128, Lb > 128 or E > 320.
 * nnr_row_dist_fwd: dist[r] = ||a[r] - b[r]||_2, aux[r] = coef * dist[r] (newsEncoders.py:391); nnr_row_dist_bwd ADDS u = gup[r] * coef *
 * (a[r] - b[r]) / dist[r] into da[r] and SUBTRACTS it from db[r] (nothing where dist[r] == 0, torch's subgradient); gup: device [n]. */
int nnr_bag_mean_fwd(const float* table, int V, int E, const int* ids_a, uint8_t* mask_a, int La, const int* ids_b, uint8_t* mask_b,
                     int Lb, int n, int separate, int act, float* out, int ldo, int off_a, int off_b, float* count, int* tok,
                     hipStream_t stream);
size_t nnr_bag_mean_bwd_ws_floats(long cap);
int nnr_bag_mean_bwd(const float* dout, int lddo, const float* out, int ldo, int off_a, int off_b, const float* count,
                     const unsigned* keys_sorted, const int* pos_sorted, long cap, int La, int Lb, int n, int V, int E, int separate,
                     int act, float* dtable_accum, float* partial_ws, hipStream_t stream);
int nnr_row_dist_fwd(const float* a, int lda, const float* b, int ldb, int n, int D, float coef, float* dist, float* aux,
                     hipStream_t stream);
int nnr_row_dist_bwd(const float* a, int lda, const float* b, int ldb, const float* dist, const float* gup, int n, int D, float coef,
                     float* da_accum, int ldda, float* db_accum, int lddb, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ KCNN / DKN (csrc/kcnn.hip)
 * The kernels around the one convolution product of the KCNN news encoder (newsEncoders.py:203-241, layers.py:47-79 `naive`): n titles of L
 * positions, E = word_embedding_dim, C = cnn_kernel_num, window w, p = (w - 1) / 2, Lp = L + w - 1.  All fp32, no float atomics anywhere.
 * nnr_kcnn_image_fwd: the padded image Xp [n][Lp][3][E] = the A operand of the convolution (the window of output position t is the 3 w E
 *   floats from padded row t on: a product with lda = 3 E < K = 3 w E).  Rows [0, p) and [p + L, Lp) of every title are written as zero;
 *   row p + t holds [word_table[text[i, t]] | tanh(pre1[i, t]) | tanh(pre2[i, t])] (text int32 [n, L], an id outside [0, V): a zero row;
 *   pre1 / pre2 [n * L, E]: the projected entity / context rows before the tanh).  16-byte accesses when E % 4 == 0 and every base is
 *   16-byte aligned, scalar ones otherwise.
 * nnr_kcnn_image_bwd: from dXp and Xp (both [n][Lp][3][E]) the compact [n * L, E] arrays dx0 = channel 0 of dXp, dpre1 = channel 1 *
 *   (1 - x1^2), dpre2 likewise; halo rows are not read.
 * nnr_window_max_fwd: z [n * Lp rows, row stride ldz >= C] = the raw convolution rows (no bias yet; row i * Lp + t = output position t of
 *   title i), bias [C].  out[i, c] = max(0, max over t in [0, L - w + 1) of fl(z + bias[c])) -- relu, then the maximum over the first
 *   L - w + 1 positions only (layers.py:77-78) --, arg[i, c] (uint8) = the LOWEST t that attains a positive maximum, 255 when there is none.
 * nnr_window_max_bwd: dz [lead_rows + n * Lp, C] dense, EVERY element written once: zero in the lead_rows leading rows (the data-gradient
 *   product reads w - 1 of them), g[i, c] at row lead_rows + i * Lp + arg[i, c], zero elsewhere (also in the rows the maximum never sees).
 *   db [C] is WRITTEN (not added to): the sum of g[i, c] over the titles with arg != 255 in a fixed order (groups of 8 titles, then the
 *   groups in order): same inputs, same bits.  ws: nnr_window_max_bwd_ws_floats(n, C) floats owned by the calling stream.
 * The operand layouts of the Conv2d weight W [C][E][w][3] are nnr_permute calls: P [C][w][3][E] = the B operand of the convolution,
 *   Q [3][E][w][C] with the window reversed (Q[j][e][k][c] = W[c][e][w-1-k][j]) = the B operand of the data gradient dXp = dz . W (A = dz
 *   with lda = C < K = w C), and W.grad += the gradient of P.
 * NNR_ERR_UNSUPPORTED when L + w - 1 > 255, w > 8, E > 1024 or L < w (the reference's slice is empty there). */
int nnr_kcnn_image_fwd(const float* word_table, int V, const int* text, const float* pre1, const float* pre2, int n, int L, int E, int w,
                       float* Xp, hipStream_t stream);
int nnr_kcnn_image_bwd(const float* dXp, const float* Xp, int n, int L, int E, int w, float* dx0, float* dpre1, float* dpre2,
                       hipStream_t stream);
int nnr_window_max_fwd(const float* z, int ldz, const float* bias, int n, int C, int L, int w, float* out, uint8_t* arg,
                       hipStream_t stream);
size_t nnr_window_max_bwd_ws_floats(int n, int C);
int nnr_window_max_bwd(const float* g, const uint8_t* arg, int n, int C, int L, int w, int lead_rows, float* dz, float* db, float* ws,
                       hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ NAML view attention (csrc/naml.hip)
 * The multi-view attention of the NAML family (variantEncoders.py:139-142): out[i] = sum over the V = Vt + 2 views of softmax_v(score_v[i]) *
 * row_v[i] for n news of C floats.  Views in order: Vt text views (t0, and t1 when Vt == 2: rows [n, C], scores [n]), then two TABLE views
 * A and B given as (rows [R, C], score [R], ids int32 [n]) -- news i takes row ids[i]; an id outside [0, R) reads row 0 and sends no
 * gradient.  All fp32, no float atomics.
 * nnr_view_pool_fwd: alpha [n, V] (the softmax weights, the maximum subtracted) and out [n, C] are written.  t1 / ts1 are ignored for Vt == 1.
 * nnr_view_pool_bwd: from dout [n, C]: dt_v [n, C] = alpha_v dout and dts_v [n] = ds_v = alpha_v (<dout, row_v> - sum_u alpha_u <dout, row_u>)
 *   for the text views; for a table view drows [R, C] = the sum of alpha_v dout, and dscore [R] the sum of ds_v, over the news with that id
 *   in ascending news order inside four fixed quarters of the news list (same inputs, same bits); a table row without news gets zeros.
 *   All eight outputs are WRITTEN.  ws: 2 n floats owned by the calling stream.
 * NNR_ERR_UNSUPPORTED for a non-positive n, C, Ra or Rb and for Vt outside 1..2. */
int nnr_view_pool_fwd(const float* t0, const float* ts0, const float* t1, const float* ts1, int Vt, const float* rowsA, const float* scoreA,
                      const int* idsA, int Ra, const float* rowsB, const float* scoreB, const int* idsB, int Rb, int n, int C, float* alpha,
                      float* out, hipStream_t stream);
int nnr_view_pool_bwd(const float* dout, const float* t0, const float* t1, int Vt, const float* rowsA, const int* idsA, int Ra,
                      const float* rowsB, const int* idsB, int Rb, const float* alpha, int n, int C, float* dt0, float* dts0, float* dt1,
                      float* dts1, float* drowsA, float* dscoreA, float* drowsB, float* dscoreB, float* ws, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ padded-row Conv1d image (csrc/naml.hip)
 * The kernels around the ONE product of Conv1d(E -> C, window k, padding (k - 1) / 2) over n news of L positions (Lp = L + k - 1):
 * nnr_conv1d_image_fwd: Xp [n][Lp][E], every element written by this launch: rows [0, (k - 1) / 2) and [(k - 1) / 2 + L, Lp) of a news are
 *   zero, row (k - 1) / 2 + t holds dropout(word_table[text[i, t]]) (text int32 [n, L]; an id outside [0, V): a zero row).  The keep-mask is
 *   keyed on the compact index (i L + t) E + e: bit for bit nnr_embed_gather's for the same p and seed on the un-padded [n L, E] rows.
 *   The window of output position t is the k E floats from padded row t on: a product with lda = E < K = k E over M = n Lp - (k - 1) rows.
 * nnr_conv1d_dz_pad: dz [(k - 1) + n Lp][C], every element written: row (k - 1) + i Lp + t = (y > 0 ? dy : 0) of the compact row i L + t for
 *   t < L (y: the compact relu output or anything with its sign, e.g. its dropped copy), zero in the k - 1 leading rows and at t >= L.
 * nnr_conv1d_image_bwd: dx [n L, E] = the keep-mask (same key, p, seed as forward) times row i Lp + (k - 1) / 2 + t of dXp [n Lp, E].
 * NNR_ERR_UNSUPPORTED for a non-positive dimension, an even k and k > 8. */
int nnr_conv1d_image_fwd(const float* word_table, int V, const int* text, int n, int L, int E, int k, float p, uint32_t seed, float* Xp,
                         hipStream_t stream);
int nnr_conv1d_dz_pad(const float* dy, const float* y, int n, int L, int C, int k, float* dz, hipStream_t stream);
int nnr_conv1d_image_bwd(const float* dXp, int n, int L, int E, int k, float p, uint32_t seed, float* dx, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ HDC (csrc/hdc.hip)
 * The kernels around the dilated convolutions of the HDC news encoder (newsEncoders.py:244-278), which run as accumulating products of
 * nnr_gemm_f32.  Activations are position-major: n news of S = L + 2 rows (category row, subCategory row, L title word rows) of C floats,
 * compact [n][S][C] or padded [n][S + 2 pad][C] with `pad` zero halo rows on both sides of every news.  All fp32, no float atomics.
 * nnr_hdc_seq_fwd: d0 [n][S][E] and d0p [n][S + 2 pad][E] from the three tables (text int32 [n, L], category / subCategory int32 [n]; an id
 *   outside its table: a zero row); tok_word / tok_cat / tok_sub int32 [n S]: the id at the rows that came from that table, -1 elsewhere
 *   (sorted by nnr_token_sort they are the occurrence lists of the three table gradients).
 * nnr_hdc_ln_relu_fwd: LayerNorm([F, S]) + ReLU per news.  z: z_rows >= S rows of F floats per news, rows [0, S) are read; mean and
 *   variance over all S F values (two passes), gamma / beta [F][S] read in place; y [n][S][F]; y_padded (optional) [n][S + 2 pad][F] with
 *   zero halo rows; stats [n][2] = mean, 1 / sqrt(var + eps).
 * nnr_hdc_ln_relu_bwd: IN PLACE on z: rows [0, S) of every news become the gradient of the LayerNorm input, rows [S, z_rows) zero;
 *   dgamma / dbeta [F][S] += sums over the news in a fixed order (partials of 32 news in ws, nnr_hdc_ln_bwd_ws_floats floats).
 * nnr_hdc_unpad_add: out [n][S][C] = a [n][S][C] (may be NULL) + rows [pad, pad + S) of b_padded [n][S + 2 pad][C].
 * The tap-major form P [w][F] (rows of ldp >= C floats, C used) of a Conv1d weight W [F][C][w], and W.grad += the gradient of P, are
 *   nnr_permute calls. */
int nnr_hdc_seq_fwd(const float* word_table, int V, const float* cat_table, int ncat, const float* sub_table, int nsub, const int* text,
                    const int* category, const int* subCategory, int n, int L, int E, int pad, float* d0, float* d0p, int* tok_word,
                    int* tok_cat, int* tok_sub, hipStream_t stream);
int nnr_hdc_ln_relu_fwd(const float* z, int z_rows, const float* gamma, const float* beta, int n, int S, int F, float eps, float* y,
                        float* y_padded, int pad, float* stats, hipStream_t stream);
size_t nnr_hdc_ln_bwd_ws_floats(int n, int S, int F);
int nnr_hdc_ln_relu_bwd(const float* dy, const float* y, float* z, int z_rows, const float* stats, const float* gamma, int n, int S, int F,
                        float* dgamma_accum, float* dbeta_accum, float* ws, hipStream_t stream);
int nnr_hdc_unpad_add(const float* a, const float* b_padded, int n, int S, int pad, int C, float* out, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ FIM (csrc/fim.hip)
 * Conv3d(Cin -> Cout, kernel K^3) + bias + ELU + MaxPool3d(size P, stride St) in one launch (userEncoders.py:257-260); the dense
 * convolution output is never stored.  The input is addressed through strides in floats: element (image, channel, depth, row, column) at
 * image sxi + channel sxc + depth sxd + row sxh + column sxw.  Pooled sizes per axis: (in - K + 1 - P) / St + 1; convolution positions
 * that no pool cell reads are not computed.  y / arg: [imgs][PD][PH][PW][Cout] (cf_out == 0) or [imgs][Cout][PD][PH][PW] (cf_out == 1);
 * y = elu(maximum of the cell), arg (uint8) = (depth offset P + row offset) P + column offset of the LOWEST position in that scan order
 * that attains it (positions with equal windows give equal bits).
 * wp / wq, of W [Cout][Cin][K][K][K]: [Cin][K^3][Cout rounded up to 4] (the forward operand) / [Cout][K^3][Cin rounded up to 4] (the
 *   input-gradient operand), 16-byte aligned, pad entries zero (nnr_permute into a zeroed buffer).
 * nnr_conv3d_pool_bwd: g = dy (1 if y > 0 else y + 1) reaches the one position arg names.  dw_accum [Cout][Cin][K^3] and db_accum [Cout]
 *   += per-workgroup partials (ws, nnr_conv3d_pool_bwd_ws_floats floats) added in workgroup order; dx (same strides as x; may be NULL)
 *   is written once per element by a gather.  No float atomics: the same bits on every run.
 * NNR_ERR_UNSUPPORTED (nothing written) when K > 4, P > 4, St < P (overlapping windows), an axis is left without a pool cell, or the
 * staged slab (Cin K^3 Cout weights + one row of cells) exceeds 160 KB of LDS. */
int nnr_conv3d_pool_dims(int Cin, int D, int H, int W, int Cout, int K, int P, int St, int* PD, int* PH, int* PW);
int nnr_conv3d_pool_fwd(const float* x, long sxi, long sxc, long sxd, long sxh, long sxw, const float* wp, const float* bias, int imgs,
                        int Cin, int D, int H, int W, int Cout, int K, int P, int St, int cf_out, float* y, uint8_t* arg,
                        hipStream_t stream);
size_t nnr_conv3d_pool_bwd_ws_floats(int imgs, int Cin, int D, int H, int W, int Cout, int K, int P, int St);
int nnr_conv3d_pool_bwd(const float* dy, const float* y, const uint8_t* arg, const float* x, long sxi, long sxc, long sxd, long sxh,
                        long sxw, const float* wq, int imgs, int Cin, int D, int H, int W, int Cout, int K, int P, int St, int cf_out,
                        float* dx, float* dw_accum, float* db_accum, float* ws, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ device-resident corpus
 * (SURVEY.md section 8 f-1 / f-2).  The corpus tables MIND_Corpus builds (MIND_corpus.py:261-268, 336-353) live in HBM;
 * a training batch is described by behaviour indices + the (1 + K) sampled news ids of each behaviour.
 * nnr_corpus_batch   = MIND_Train_Dataset.__getitem__ + default collate (MIND_dataset.py:70-76): fills the 21 batch tensors
 *                      (dtypes of the reference's DataLoader: int64 user ids / cluster indices, int32 ids, 1-byte bools, fp32 graph).
 *                      With graph_table == NULL the graph / cluster mask / cluster indices are left to nnr_history_graph.
 * nnr_history_graph  = MIND_Corpus.preprocess step 6 (MIND_corpus.py:162-221) for a batch, from the history's category ids:
 *                      norm 0 = none, 1 = symmetric D^-1/2 A D^-1/2, 2 = asymmetric D^-1 A (self connections on), 3 = none and
 *                      NO self connections (--no_self_connection; the reference asserts it excludes normalisation,
 *                      config.py:56,111).  Bit-identical to the numpy result. */
typedef struct nnr_corpus_tables {
  const int* news_category; const int* news_subCategory;                       /* [news] */
  const int* title_text; const uint8_t* title_mask; const int* title_entity;   /* [news, T] */
  const int* abstract_text; const uint8_t* abstract_mask; const int* abstract_entity;   /* [news, C] */
  const long* beh_user; const int* beh_history; const uint8_t* beh_history_mask; const int* beh_line;   /* [behaviours(, H)] */
  const float* graph_table; const uint8_t* cmask_table; const long* cidx_table;   /* optional [lines, G, G] / [lines, K1] / [lines, H] */
  int T, C, H, G, K1;                                                          /* G = H + category_num, K1 = category_num + 1 */
} nnr_corpus_tables;
typedef struct nnr_batch_out {                                                 /* the 21 tensors, argument order of trainer.py:105-106 */
  long* user_id;
  int* u_cat; int* u_sub; int* u_tt; uint8_t* u_tm; int* u_te; int* u_ct; uint8_t* u_cm; int* u_ce;
  uint8_t* u_hmask; float* u_graph; uint8_t* u_cmask; long* u_cidx;
  int* n_cat; int* n_sub; int* n_tt; uint8_t* n_tm; int* n_te; int* n_ct; uint8_t* n_cm; int* n_ce;
} nnr_batch_out;
int nnr_corpus_batch(const nnr_corpus_tables* t, const nnr_batch_out* o, const int* beh_idx, const int* samples, int ld_samples, int B,
                     int S, hipStream_t stream);
int nnr_history_graph(const int* cats, const uint8_t* hmask, int B, int H, int K, int norm, float* graph, uint8_t* cmask, long* cidx,
                      hipStream_t stream);
/* Negative sampling (the rule of MIND_Train_Dataset.negative_sampling, MIND_dataset.py:27-47) as a pure
 * function of (seed, epoch, behaviour): ranks agree without talking, any subset of rows can be redrawn, and the table is rewritten
 * in place.  clicks [behaviours]; neg_offsets [behaviours + 1] indexes neg_ids (CSR: behaviour b's non-clicked news are
 * neg_ids[neg_offsets[b] .. neg_offsets[b + 1]), m of them, 1 <= m < 2^31); beh_idx: the n behaviours to draw, NULL = 0 .. n - 1.
 * Row b is written at samples + b * ld_samples, whichever way it was named: column 0 = clicks[b], columns 1 .. K as follows, columns
 * beyond 1 + K untouched.
 *   m <= K : column j + 1 = list[j % m] (exact, no randomness).
 *   m >  K : the list's entries at K pairwise distinct POSITIONS, uniform over ordered K-tuples of positions, by a partial
 *            Fisher-Yates walk over the virtual array a[p] = p: for j = 0 .. K - 1, p = j + bounded(r_j, m - j), column j + 1 =
 *            list[a[p]], then a[p] = a[j] (the at most K displaced entries live in registers).  No rejection loop: every loop has at
 *            most K trips.
 *   With H = the lowbias32 finaliser (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16) and every sum and
 *   product taken mod 2^32:   key = H(seed ^ H(epoch + 0x9E3779B9)),   r_j = H(H(b ^ key) + j * 0x9E3779B9 + 1),
 *   bounded(r, range) = (uint64(r) * range) >> 32, whose relative bias is at most range / 2^32.  Two chained rounds per draw: a single
 *   hash of a structured counter fails a per-column chi-square at list lengths >= 1000 (tests/test_negsample_host.py gates this one).
 * NNR_ERR_UNSUPPORTED for K outside 1 .. 16; NNR_ERR_ARG for ld_samples < 1 + K, n < 1 or a null table; nothing is written then.
 * A list of length 0 is the caller's to refuse (the reference divides by zero there); such a row is left untouched. */
int nnr_negative_sample(const int* clicks, const long* neg_offsets, const int* neg_ids, const int* beh_idx, int n, int K, uint32_t seed,
                        int epoch, int* samples, int ld_samples, hipStream_t stream);
/* Listwise evaluation: the click scores of n (impression, candidate) samples against a user table that was
 * encoded once per impression (or once per row of K candidates):
 *   scores[j] = sum_d user[row[j] * ldu + d] * reps[cand[j] * ldr + d]      for j < n.
 * user [n_user, D] with row stride ldu >= D, reps [n_reps, D] with row stride ldr >= D (the table of distinct news representations),
 * row / cand int32 [n], scores float [n]; entries of scores beyond n are not touched.  Summation order: one wave per sample; lane l
 * accumulates d = l, l + 64, ... in ascending order with fmaf from 0, then the 64 lane sums are folded by a butterfly (partner l ^ 32,
 * l ^ 16, ..., l ^ 1, each step v += partner's v).  16-byte loads when D, ldu and ldr are multiples of 4 and both tables are 16-byte
 * aligned, 4-byte loads otherwise, in the same order: a sample's score is a pure function of its two rows, to the bit, wherever it
 * stands and whichever path the launch took.  No atomics, no LDS.
 * NNR_ERR_ARG for a null pointer, n < 1, D < 1, ldu < D, ldr < D, n_user < 1 or n_reps < 1; nothing is launched then.  The indices
 * are trusted: row[j] in 0 .. n_user - 1 and cand[j] in 0 .. n_reps - 1 are the caller's to check (ops.list_scores does). */
int nnr_list_scores(const float* user, long n_user, int ldu, const float* reps, long n_reps, int ldr, const int* row, const int* cand,
                    long n, int D, float* scores, hipStream_t stream);
/* Top-K recommendation: for every user row the K eligible news rows of the largest inner products, without a
 * [n_user, n_reps] score buffer.  user [n_user, D] with row stride ldu >= D, reps [n_reps, D] with row stride ldr >= D.  News row r is
 * ELIGIBLE for user u when (valid is NULL or valid[r] != 0) and r does not occur in exclude[u * ld_ex + 0 .. E) (exclude NULL or E = 0:
 * no list; entries outside 0 .. n_reps - 1 are ignored, so -1 pads a list; duplicates are allowed).
 *   score(u, r) = sum_d user[u * ldu + d] * reps[r * ldr + d]
 * idx [n_user, K] / score [n_user, K]: the eligible rows of the largest scores, by score descending, equal scores by ascending row,
 * ties at the cut broken the same way; score[u, k] is the value computed for idx[u, k].  With fewer than K eligible rows the tail is
 * idx = -1, score = -inf.  The inputs are finite by contract (a NaN or an infinity in either table makes the order undefined).
 * Summation order: ONE chain  acc = fmaf(user[u, d], reps[r, d], acc)  over d = 0, 1, .., D - 1 from acc = +0 (the exact-fp32 matrix
 * instruction v_mfma_f32_32x32x2_f32 is this chain, two steps per instruction; the zero-filled tail of the last slab of 32 leaves it as it
 * is).  So score(u, r) is a pure function of the two rows, to the bit, wherever they stand in their tables and whatever n_user, n_reps, the
 * strides, the alignment (16-byte loads when D, ldu and ldr are multiples of 4 and both tables are 16-byte aligned, 4-byte loads otherwise)
 * and the number of news splits of the launch; the selection is a function of the scores and rows alone.  No atomics, no order that depends
 * on which workgroup finishes first.  Launches with few user rows split the news over several workgroups per 64 users, which leave
 * partial lists [n_user, splits, K] in `workspace`; a second launch merges them.  nnr_topk_workspace_bytes (host only, no launch) is the
 * size that needs, 0 when the launch does not split (workspace may be NULL then) and 0 for sizes nnr_topk_scores refuses.
 * NNR_ERR_UNSUPPORTED for K > 64 (a list is one entry per lane) or n_reps >= 2^31.  NNR_ERR_ARG, with nothing launched, for a null user,
 * reps, idx or score, n_user < 1, n_reps < 1, D < 1, K < 1, ldu < D, ldr < D, E < 0, ld_ex < E, E > 0 with a null list, or a workspace that
 * is smaller than nnr_topk_workspace_bytes says (or null, or not 4-byte aligned, when that is not 0). */
size_t nnr_topk_workspace_bytes(long n_user, long n_reps, int K);
int nnr_topk_scores(const float* user, long n_user, int ldu, const float* reps, long n_reps, int ldr, int D, const uint8_t* valid,
                    const int* exclude, int E, int ld_ex, int K, int* idx, float* score, void* workspace, long workspace_bytes,
                    hipStream_t stream);
/* Full-pool ranks: where named news rows (targets) land when a user's whole pool is ranked, without a
 * [n_user, n_reps] score buffer.  user, reps, valid and exclude are nnr_topk_scores' (above), with its eligibility rule and its score.
 * t_off int32 [n_user + 1], ascending, t_off[0] = 0, t_off[n_user] = n_target; t_news int32 [n_target]: entries t_off[u] .. t_off[u + 1] - 1
 * are the targets of user row u, given as rows of reps.  A user may have none, many, or one twice.
 *   t_score[j]   = score(u, t_news[j]), the chain  acc = fmaf(user[u, d], reps[t, d], acc)  over d ascending from +0, computed on its own
 *                  by a pre-pass; it has the bits of the value the tile walk computes for that pair (and nnr_topk_scores returns);
 *   pool_size[u] = the number of rows eligible for u;
 *   ahead[j]     = the number of eligible rows r with score(u, r) > t_score[j], or score(u, r) == t_score[j] and r < t_news[j]: the number
 *                  of entries nnr_topk_scores places before the target (its position in an unbounded list); -1 when the target is itself
 *                  ineligible for its user (valid == 0, or in the user's exclusion list).
 * The inputs are finite by contract; a score that overflows to -inf counts as ineligible in pool_size.  Integer counts of exact
 * comparisons: nothing depends on n_user, n_reps, the strides, the load path or the number of news splits.  No atomics: a counter belongs
 * to the one wave that owns its user.  Launches with few user rows split the news as nnr_topk_scores does and leave partial counts
 * [n_target + n_user, splits] int32 in `workspace`; a second launch adds them in split order.  nnr_pool_rank_workspace_bytes (host only) is
 * that size, 0 when the launch does not split (workspace may be NULL then) and 0 for sizes nnr_pool_ranks refuses.
 * NNR_ERR_ARG, with nothing launched, for a null user, reps, t_off or pool_size, n_user < 1, n_reps < 1, D < 1, ldu < D, ldr < D, E < 0,
 * ld_ex < E, E > 0 with a null list, n_target < 0, n_target > 0 with a null t_news, ahead or t_score, or a workspace that is smaller than
 * the query says (or null, or not 4-byte aligned, when that is not 0).  NNR_ERR_UNSUPPORTED for 2^31 - 1 user rows and more, n_reps or
 * n_target >= 2^31, or a grid beyond 2^31 - 1 workgroups.  t_off and t_news are trusted (ops.pool_ranks checks them), but no access leaves
 * the tables whatever they hold: offsets are clamped into 0 .. n_target, and a target outside 0 .. n_reps - 1 reports ahead = -1 and a NaN score. */
size_t nnr_pool_rank_workspace_bytes(long n_user, long n_reps, long n_target);
int nnr_pool_ranks(const float* user, long n_user, int ldu, const float* reps, long n_reps, int ldr, int D, const uint8_t* valid,
                   const int* exclude, int E, int ld_ex, const int* t_off, const int* t_news, long n_target, int* ahead, float* t_score,
                   int* pool_size, void* workspace, long workspace_bytes, hipStream_t stream);
/* The archive form of the two entry points above: a user row is A vectors ("archives", 1 <= A <= 16) and the score of a
 * pair is their softmax-weighted inner product with the news row, OMAP's click score (userEncoders.py:367-369).  user [n_user][A][D]: archive
 * a of user u starts at user + u * ldu + a * lda, lda >= D, ldu >= (A - 1) * lda + D.  Everything else -- reps, valid, exclude, the
 * eligibility rule, the -inf masking, the order, the tie rule, the -1 / -inf tail, t_off, t_news, ahead, pool_size, the workspace (its size
 * does not depend on A: nnr_topk_workspace_bytes / nnr_pool_rank_workspace_bytes) and the splits -- is the plain entry point's, applied to
 *   s_a   = the chain  acc = fmaf(user[u, a, d], reps[r, d], acc)  over d ascending from +0           (nnr_topk_scores' score of archive a)
 *   score = combine(s_0 .. s_{A-1}; scale) = sum_a w_a s_a,  w = softmax_a(scale * s_a).
 * combine, THE operation sequence (every operation fp32, rounded to nearest once; fma = one rounding; nothing is contracted or reordered):
 *   m = s_0;  den = 1;  num = s_0;                                             the state after archive 0
 *   for a = 1 .. A - 1, with s = s_a:
 *     up = (scale < 0 ? s < m : s > m)                                         s is the new extreme: the state is rescaled to it
 *     e  = expf(scale * (up ? m - s : s - m))                                  the argument is never positive: no overflow; expf is the
 *                                                                              runtime's, at most 2 ulp (1 ulp as documented for the device)
 *     up:      den = fma(den, e, 1);  num = fma(num, e, s);  m = s
 *     not up:  den = fma(1, e, den);  num = fma(s, e, num)                     (= den + e, and num + s e with one rounding)
 *   score = num / den                                                          ONE correctly rounded division
 * m is the running extreme of the archives seen so far (the maximum for scale >= 0), which is the maximum that is subtracted; den and num
 * are the softmax sums over a ascending, relative to it.  One __device__ function states this sequence; the tile walk (per accumulator
 * element, one pass over the news tile per archive) and the target pre-pass of nnr_pool_archive_ranks both call it.  So the combined score is
 * a pure function of the A + 1 rows and scale, to the bit: wherever the rows stand, whatever the strides, the load path (16-byte loads need
 * lda a multiple of 4 too), the number of news splits, and whether the tile walk or the pre-pass computed it.  Three consequences:
 *   A = 1: score = s_0 / 1, the bits of nnr_topk_scores for the same rows;
 *   scale = 0: every e is 1, den = A, score = (s_0 + .. + s_{A-1}) / A summed in ascending a;
 *   all A archives of a user equal and A in {2, 4}: num = A s_0 exactly, score = s_0.
 * The scores s_a are finite by contract, as the tables are.
 * NNR_ERR_ARG, with nothing launched, for everything the plain entry point refuses so and for A < 1, lda < D, ldu < (A - 1) * lda + D or a
 * scale that is not finite.  NNR_ERR_UNSUPPORTED for A > 16 (csrc/omap.hip's own limit on its archives) and for the plain entry point's cases. */
int nnr_topk_archive_scores(const float* user, long n_user, int ldu, int A, int lda, float scale, const float* reps, long n_reps, int ldr,
                            int D, const uint8_t* valid, const int* exclude, int E, int ld_ex, int K, int* idx, float* score, void* workspace,
                            long workspace_bytes, hipStream_t stream);
int nnr_pool_archive_ranks(const float* user, long n_user, int ldu, int A, int lda, float scale, const float* reps, long n_reps, int ldr, int D,
                           const uint8_t* valid, const int* exclude, int E, int ld_ex, const int* t_off, const int* t_news, long n_target,
                           int* ahead, float* t_score, int* pool_size, void* workspace, long workspace_bytes, hipStream_t stream);
/* De-duplicated evaluation of the rank-pairing CNE encoders: the pairing plan of every encoder call of a range of
 * reference batches, in one launch.  The reference scores dev samples in batches of batch_size consecutive samples (the last one short) and
 * runs two encoder calls per batch of b samples: the candidate call over the b sequences cand[s] and the history call over the b * H
 * sequences beh_history[s, h], sequence index s * H + h.  Inside a call it sorts the sequences by title length and by content length,
 * descending, equal lengths in ascending sequence index (torch.sort(descending=True, stable=True)), and gates the title at title-rank r with
 * the content memory at content-rank r and the content at content-rank r with the title memory at title-rank r.  For sequence i of a call,
 *   pc(i) = order_c[rank_t[i]]   the sequence whose content memory gates title i,
 *   pt(i) = order_t[rank_c[i]]   the sequence whose title memory gates content i,
 * and this entry point writes the NEWS of pc(i) and pt(i) for every sequence of every call of the samples first .. first + count - 1:
 *   pc_hist / pt_hist [count, H] and pc_cand / pt_cand [count], row j = sample first + j.
 * beh_history int32 [n, H], cand int32 [n], tlen / clen int32 [n_news]: a news' title / content length (ones of its mask with position 0
 * forced to 1), 0 .. 255.  The range's batches must be the reference's: first is a multiple of batch_size, and the range ends at a batch
 * boundary or at sample n.  tmp: count * (H + 1) * 2 ints of workspace.  One workgroup of two waves per call, one wave per stream: a counting sort over the 256 length bins whose rank inside a
 * bin is a prefix count in sequence order (a ballot per length bit, the population count of the lower lanes); integer work only, no atomics:
 * the output is a pure function of the inputs, to the bit.
 * NNR_ERR_ARG for a null pointer, H < 1, batch_size < 1, count < 1, first < 0, first % batch_size != 0, first + count > n, a range that
 * ends inside a batch or n_news < 1; nothing is launched then.  A news id outside 0 .. n_news - 1 counts as length 0 and a length is clamped to 0 .. 255, so no access leaves
 * the tables; both are the caller's to refuse (ops.cne_pair_triples does). */
int nnr_cne_pair_triples(const int* beh_history, const int* cand, const int* tlen, const int* clen, long n, int H, int n_news, int batch_size,
                         long first, long count, int* pc_hist, int* pt_hist, int* pc_cand, int* pt_cand, int* tmp, hipStream_t stream);
/* Evaluation tail: util.py:50-59 (per-impression ranks by descending score, ties in file order) +
 * evaluate.py:8-29,76-81 (AUC, MRR, nDCG@5, nDCG@10 per impression, float64).  offsets [n_impressions + 1] delimit the
 * (contiguous) candidates of each impression; per_impression [n_impressions, 4]; NaN row for a single-class impression. */
int nnr_rank_metrics(const float* scores, const uint8_t* labels, const long* offsets, int n_impressions, int* ranks,
                     double* per_impression, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ click predictor, loss, optimiser */
int nnr_logits_loss_fwd(const float* user, const float* cand, int B, int N, int D, float* logits, float* loss, float* dlogits,
                        hipStream_t stream);                                     /* model.py:126-127, trainer.py:64-66 */
int nnr_logits_fwd(const float* user, const float* cand, int B, int N, int D, float* logits, hipStream_t stream);   /* model.py:127 */
int nnr_nls_loss(const float* logits, int B, int N, float* loss, float* dlogits, hipStream_t stream);               /* trainer.py:64-66 */
int nnr_logits_bwd(const float* dlogits, const float* user, const float* cand, int B, int N, int D, float* duser, float* dcand,
                   int dcand_accumulate, hipStream_t stream);
/* --gcn_layer_norm (config.py:61; layers.py:273-274,287-288): nn.LayerNorm([D]) between the graph convolution and the ReLU,
 * fused with the rest of GCNLayer.forward / GCN.forward:  y = dropout(relu(LN(u) * gamma + beta) + resid)  (resid may be NULL,
 * p may be 0).  xhat [rows, D], rstd [rows] and r_out = relu(.) [rows, D] are saved for the backward pass; D <= 1024.
 * Backward: du = d(LN input) from dv = d(LN output); dgamma / dbeta are ACCUMULATED (f32 atomics). */
int nnr_layernorm_fwd(const float* u, const float* gamma, const float* beta, float eps, long rows, int D, float* xhat, float* rstd,
                      float* r_out, const float* resid, float* y, float p, uint32_t seed, hipStream_t stream);
int nnr_layernorm_bwd(const float* dv, const float* xhat, const float* rstd, const float* gamma, long rows, int D, float* du,
                      float* dgamma, float* dbeta, hipStream_t stream);
/* *out = sum g^2 (stored), a DETERMINISTIC function of g (fixed-order two-level sum: data-parallel ranks must clip by the same bits);
 * launches of one process must be stream-ordered (one device-global scratch) */
int nnr_sumsq(const float* g, long n, float* out, hipStream_t stream);
/* The same over one SPAN of the gradient, chained: *out = sum g^2 + (add_in ? *add_in : 0), fixed order.  `slot` (0..3) selects the scratch
 * set: launches that may run concurrently (different streams) must use different slots; nnr_sumsq uses slot 0.  Round 5: the norm of the
 * word-embedding table's gradient (70 % of the floats) is taken on a helper stream as soon as its last scatter is done, beside the LSTM
 * weight-gradient GEMMs of the step's tail, and only the remaining spans are summed on the optimizer's stream (trainer.py:118). */
int nnr_sumsq_part(const float* g, long n, float* out, const float* add_in, int slot, hipStream_t stream);
/* clip_grad_norm_(max_norm = clip) + torch.optim.Adam step on one flat buffer (trainer.py:118-120); grads are scaled by
 * grad_scale first (1/world_size after the RCCL sum all-reduce).  A step whose squared gradient norm is not finite is
 * skipped as a whole (parameters and moments untouched). */
int nnr_clip_adam(float* p, const float* g, float* m, float* v, long n, const float* sumsq, float grad_scale, float clip, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, hipStream_t stream);

/* Steps nnr_clip_adam skipped so far in this process (non-finite gradient norm: overflow, or the NaN poison of a timed-out recurrence
 * exchange).  The reference would go visibly NaN there (trainer.py:118-120); here the step is dropped and COUNTED -- poll this every few
 * hundred steps (synchronous device read); reset != 0 clears the counter. */
int nnr_adam_skipped_steps(unsigned* host_out, int reset);
/* The same count WITHOUT a synchronisation: nnr_clip_adam's kernel mirrors it into pinned, device-mapped host memory, so the value covers
 * every optimizer step that has completed on the device.  Cheap enough to read after every step (Trainer.train_step does; with an event
 * wait every NNR_SKIP_POLL-th step that bounds how far the host runs ahead, a skipped step is reported within 2 x NNR_SKIP_POLL steps). */
int nnr_adam_skipped_peek(unsigned* host_out);

/* ------------------------------------------------------------------------------------------------ data parallelism (RCCL over xGMI)
 * Replaces DistributedDataParallel's gradient all-reduce / parameter broadcast (trainer.py:212-219,297): one communicator per
 * process = per GPU, ONE in-place fp32 sum all-reduce of the flat gradient buffer per step; the 1/world average is folded into
 * nnr_clip_adam.  RCCL is resolved at run time from the copy already loaded in the process (PyTorch-ROCm's).  Rank 0 creates
 * the 128-byte id and the launcher distributes it (any side channel: the torchrun store, a file, MPI). */
typedef struct nnr_dp_ctx nnr_dp_ctx;
int nnr_dp_unique_id(void* out128);
int nnr_dp_init(const void* uid128, int rank, int world, nnr_dp_ctx** ctx);          /* binds to the current HIP device */
int nnr_dp_allreduce(nnr_dp_ctx* ctx, float* flat, size_t n, hipStream_t stream);
int nnr_dp_broadcast(nnr_dp_ctx* ctx, float* flat, size_t n, int root, hipStream_t stream);
int nnr_dp_destroy(nnr_dp_ctx* ctx);
/* Test hook for boxes with ONE GPU (RCCL refuses two ranks on one device): from now on every nnr_dp_allreduce of `ctx` behaves as if
 * `ranks` ranks held the SAME buffer -- the sum is ranks x the local values (a scale kernel on the same stream right behind the
 * collective, so it is part of whatever launch sequence the all-reduce is part of, recorded tapes included).  With a power of two the
 * result is exact, and a bucket that was NOT exchanged shows as 1 x instead of ranks x its gradient (tests/test_hip_dp_gpu.py:
 * the C-ABI binding + touched-row exchange over replayed steps).  ranks = 1 turns it off.  Never set by the product path. */
int nnr_dp_emulate_ranks(nnr_dp_ctx* ctx, int ranks);
/* Diagnostics: a stand-in for RCCL's RESIDENT ring kernels on a box with one GPU -- `workgroups` x 512 threads sweep their slice of buf
 * [n] `iters` times (read-modify-write through HBM), occupying as many CU slots for the duration.  The co-residency soak of the CU-pair
 * recurrence (tests/test_hip_dp_gpu.py, tools/replay_soak.py --busy) runs it on a side stream beside every step. */
int nnr_dp_busy(float* buf, long n, int workgroups, int iters, hipStream_t stream);
/* Touched-row exchange of the word-embedding table's gradient (the table is 70 % of the all-reduced bytes, and only
 * the rows of words in the step's batch are non-zero; trainer.py:297 reduces all of it).  nnr_rows_touch: flags[tok[i]] = 1 for the live
 * packed rows of a token stream (flags: V floats, zeroed by the caller at the start of the step and summed over the ranks before
 * nnr_rows_compact); nnr_rows_compact: pos[w] = index of row w among the touched rows (flags[w] > 0) or -1, *count = their number;
 * nnr_rows_pack / nnr_rows_unpack: packed[pos[w], :] <-> dense[w, :] for the touched rows.  The dense gradient after unpacking equals
 * what the full all-reduce produces (untouched rows are zero on every rank), so clip + Adam stay dense and unchanged. */
int nnr_rows_touch(const int* tok, long cap, const int* n_dev, int V, float* flags, hipStream_t stream);
int nnr_rows_compact(const float* flags, int V, int* pos, int* count, hipStream_t stream);
int nnr_rows_pack(const float* dense, const int* pos, int V, int E, float* packed, hipStream_t stream);
int nnr_rows_unpack(const float* packed, const int* pos, int V, int E, float* dense, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ fused small launches (csrc/fuse.hip)
 * feature_fusion (newsEncoders.py:50-54) for the union of the candidate call (rows [0, n0), ids cat0 / sub0) and the history call
 * (rows [n0, n0 + n1), ids cat1 / sub1; n1 may be 0): out[row, 0:cd] = dropout(category row), out[row, cd:cd+sd] = dropout(subCategory
 * row); masks = nnr_small_embed_fwd's (flat index row * dim + column, one seed per table).  Backward accumulates both table gradients. */
int nnr_fusion_rows_fwd(const float* cat_table, const float* sub_table, const int* cat0, const int* sub0, int n0, const int* cat1,
                        const int* sub1, int n1, int cd, int sd, float* out, int ldo, float p, uint32_t seed_cat, uint32_t seed_sub,
                        hipStream_t stream);
int nnr_fusion_rows_bwd(const int* cat0, const int* sub0, int n0, const int* cat1, const int* sub1, int n1, int cd, int sd, const float* dout,
                        int lddo, float* dcat_table_accum, float* dsub_table_accum, float p, uint32_t seed_cat, uint32_t seed_sub,
                        hipStream_t stream);
/* The same gradients, reproducibly (one workgroup per table row scans the ids in order: no run merging, no arrival-order atomics);
 * ncat / nsub = rows of the two tables; cd, sd <= 128. */
int nnr_fusion_rows_bwd_det(const int* cat0, const int* sub0, int n0, const int* cat1, const int* sub1, int n1, int cd, int sd, int ncat,
                            int nsub, const float* dout, int lddo, float* dcat_table_accum, float* dsub_table_accum, float p,
                            uint32_t seed_cat, uint32_t seed_sub, hipStream_t stream);
/* Click predictor + loss + their backward in one launch (model.py:126-127, trainer.py:64-66): logits [B, N], loss (scalar, a fixed-order
 * mean), dlogits [B, N] (optional), duser / dcand [B, N, D] (both or neither); terms_ws: B floats of scratch.  N <= 64. */
int nnr_click_loss(const float* user, const float* cand, int B, int N, int D, float* logits, float* loss, float* dlogits, float* duser,
                   float* dcand, float* terms_ws, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ DSSM (csrc/dssm.hip)
 * The DSSM baseline of general_recommendation_methods/ (DSSM_model.py:29-36, DSSM_main.py:63).  All buffers fp32, no float atomics, same
 * inputs -> same bits.
 * Weighted bag: two streams in one launch, a (users: na rows of La positions) and b (news: nb rows of Lb positions; nb == 0: none), into
 *   one stacked out [na + nb, E].  Per stream a term-vector table ids int32 [R, L] / w f32 [R, L] and an optional row selector sel int32
 *   [n] (NULL: identity, then R >= n); a selector entry outside [0, R) selects an empty row.
 *     out[r, e] = sum_j keep(seed, (r * L + j) * E + e) * scale * w[sel[r], j] * table[ids[sel[r], j], e],  scale = 1 / (1 - p)
 *   (stream b: rows na + r, seed_b; r and j count inside the stream; keep is csrc/common.h:nnr_keep; p == 0 skips the hash).  A position
 *   with w == 0 contributes nothing and its table row is not read: the reference's 0 * row differs only for a row holding a non-finite
 *   value.  An id outside [0, V) contributes a zero row and receives no gradient.  Sum order: positions ascending inside a chunk of
 *   `chunk` positions (compensated), then the chunks ascending.  tok (optional) int32 [na * La + nb * Lb] (stream a, then stream b)
 *   receives the word id of every live position and -1 elsewhere: sorted by nnr_token_sort (n_dev = NULL) it is the backward's list.
 *   ws: nnr_wbag_fwd_ws_floats(na, La, nb, Lb, E) floats (never NULL).
 * nnr_wbag_dims (host only): the chunk length and the chunks per row of each stream; NNR_ERR_UNSUPPORTED (from the launches too, before
 *   anything is written) unless 1 <= E <= 1024, 1 <= La <= 4096 and 0 <= Lb <= 4096 (chunk is written in either case).  Any E: rows move
 *   as 16-byte vectors when E % 4 == 0, as 8-byte vectors when E % 2 == 0, as scalars otherwise.
 * Backward: dtable[word, :] += sum over the word's live occurrences, in sorted-list order, of keep * scale * w * dout[row, :], dout
 *   [na + nb, E] read through the occurrence's row: no [tokens, E] buffer.  cap = na * La + nb * Lb entries in keys_sorted / pos_sorted.
 *   One writer per table row per launch (both streams share the one list); partial_ws: nnr_wbag_bwd_ws_floats(cap, E) floats.
 * nnr_cosine_loss mirrors nnr_click_loss: user [B, F], news [B, N, F]; logits[b, n] = <u_b, v_bn> / (|u_b| |v_bn|), loss = mean_b of
 *   -log_softmax(logits)[b, 0] (a fixed-order mean), dlogits [B, N], duser [B, F] (the sum over the N candidates in ascending order),
 *   dnews [B, N, F] (duser and dnews: both or neither).  loss, dlogits, duser, dnews may all be NULL: the eval call, logits only (the
 *   same bits).  ws: B floats, needed with loss.  N > 64: NNR_ERR_UNSUPPORTED.  A zero-norm row gives NaN logits (the reference's 0 / 0);
 *   the gradients of such a sample are not specified.
 * nnr_tanh_drop_bwd: dz = mask(dy) * (1 - t * t) behind y = dropout(tanh(z)), t = tanh(z); mask keyed by the flat element index. */
int nnr_wbag_dims(int E, int La, int Lb, int* chunk, int* nchunk_a, int* nchunk_b);
size_t nnr_wbag_fwd_ws_floats(int na, int La, int nb, int Lb, int E);
int nnr_wbag_fwd(const float* table, int V, int E, const int* ids_a, const float* w_a, const int* sel_a, int Ra, int na, int La,
                 const int* ids_b, const float* w_b, const int* sel_b, int Rb, int nb, int Lb, float p, uint32_t seed_a, uint32_t seed_b,
                 float* out, int* tok, float* ws, hipStream_t stream);
size_t nnr_wbag_bwd_ws_floats(long cap, int E);
int nnr_wbag_bwd(const float* dout, const unsigned* keys_sorted, const int* pos_sorted, long cap, const float* w_a, const int* sel_a, int Ra,
                 int na, int La, const float* w_b, const int* sel_b, int Rb, int nb, int Lb, int V, int E, float p, uint32_t seed_a,
                 uint32_t seed_b, float* dtable_accum, float* partial_ws, hipStream_t stream);
int nnr_cosine_loss(const float* user, const float* news, int B, int N, int F, float* logits, float* loss, float* dlogits, float* duser,
                    float* dnews, float* ws, hipStream_t stream);
int nnr_tanh_drop_bwd(const float* dy, const float* t, float* dz, long n, float p, uint32_t seed, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------ fills / copies
 * What the host framework's fill / copy / index-put kernels did inside the step (optimizer.zero_grad() at trainer.py:116,
 * torch.cat of the two encoder calls' id tensors, `user_history_category_mask[:, -1] = 1` at userEncoders.py:73), as entry points,
 * so that a whole training step is a sequence of calls into this library (see the tape below). */
int nnr_fill_zero(void* p, size_t bytes, hipStream_t stream);
int nnr_copy_bytes(void* dst, const void* src, size_t bytes, hipStream_t stream);          /* device to device */
int nnr_fill_column_u8(uint8_t* m, int rows, int cols, int col, int value, hipStream_t stream);   /* m[:, col] = value */

/* ------------------------------------------------------------------------------------------------ launch-sequence tape
 * Replaces the per-call Python dispatch of the reference's training step (trainer.py:105-120: ~140 framework calls per step)
 * by a native replay: the host side records the entry-point calls of ONE step -- function, arguments (by-pointer structs are
 * copied), HIP stream -- plus the step's cross-stream dependencies, and replays the sequence with one call per segment
 * (csrc/tape.hip).  Every replayed call runs the real entry point above.  Per-step changes are patched in before a replay:
 * value patches (dropout seeds, Adam's step number: value[kind] + addend) and input patches (pointers into the batch tensors:
 * input[kind - 1000] + addend).  A tape owns nothing but its argument copies and events: buffers stay caller-owned and must
 * outlive it.  Not thread-safe; one tape is replayed by one host thread. */
typedef struct nnr_tape nnr_tape;
int nnr_tape_create(nnr_tape** out);
int nnr_tape_destroy(nnr_tape* t);
int nnr_tape_fn_id(const char* entry_point_name);      /* >= 0, or -1: not recordable (no stream argument / host-only query) */
int nnr_tape_fn_nargs(int fn);                         /* arguments before the trailing hipStream_t */
int nnr_tape_call(nnr_tape* t, int fn, hipStream_t stream, const uint64_t* slots, int nslots, const int* blob_slot,
                  const void* const* blob_ptr, const size_t* blob_bytes, int nblobs, int tag, size_t* slot_off_out, size_t* blob_off_out);
int nnr_tape_wait_stream(nnr_tape* t, hipStream_t waiter, hipStream_t signaller);
int nnr_tape_event_record(nnr_tape* t, uint64_t key, hipStream_t s);
int nnr_tape_event_wait(nnr_tape* t, hipStream_t s, uint64_t key);
int nnr_tape_segment(nnr_tape* t);
int nnr_tape_patch(nnr_tape* t, size_t arena_byte_off, int kind, int width, int64_t addend);
int nnr_tape_finalize(nnr_tape* t);
/* Create the HIP events of timing sets [0, nsets) ahead of a timed window of replays (host-side only, no launch). */
int nnr_tape_prepare_timing(nnr_tape* t, int nsets);
int nnr_tape_info(const nnr_tape* t, int* calls, int* ops, int* segments, int* streams, size_t* arena_bytes);
int nnr_tape_replay(nnr_tape* t, int segment, const uint64_t* values, int nvalues, const uint64_t* inputs, int ninputs, int timing_set);
int nnr_tape_timings(nnr_tape* t, int set, float* ms, int n);
int nnr_tape_timeline(nnr_tape* t, int set, float* start_ms, float* dur_ms, int* stream_idx, int n);
int nnr_tape_last_error(const nnr_tape* t, int* rc, int* call, char* name, int name_cap);

#ifdef __cplusplus
}
#endif
#endif
