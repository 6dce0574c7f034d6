"""ctypes binding of libnnr_hip.so (include/nnr_hip.h).  No torch types cross the boundary: only raw device
pointers, sizes and the HIP stream handle.  The product path has NO fallback: if the library is missing or a call
fails, an exception is raised."""
import collections
import ctypes as C
import itertools
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NNR_HIP_LIB') or os.path.join(_HERE, 'libnnr_hip.so')      # NNR_HIP_LIB: A/B a differently built library
_lib = None

vp, ci, cf, cu32, cl = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_long


class GemmArgs(C.Structure):
    _fields_ = [('A', vp), ('B', vp), ('C', vp), ('M', ci), ('N', ci), ('K', ci), ('lda', ci), ('ldb', ci), ('ldc', ci),
                ('trans_a', ci), ('trans_b', ci), ('dyn_dev', vp), ('dyn_dim', ci), ('a_idx', vp), ('b_idx', vp),
                ('drop_target', ci), ('drop_p', cf), ('drop_seed', cu32), ('drop_cols', ci), ('alpha', cf), ('bias', vp),
                ('rowvec', vp), ('ldrv', ci), ('rowvec_map', vp), ('act', ci), ('aux_out', vp), ('ldaux', ci), ('mul', vp),
                ('ldmul', ci), ('resid', vp), ('ldres', ci), ('accumulate', ci), ('atomic', ci), ('c_idx', vp),
                ('split_k', ci), ('rowdot_w', vp), ('rowdot_out', vp), ('batch', ci), ('strideA', cl), ('strideB', cl),
                ('strideC', cl), ('stride_aux', cl), ('stride_res', cl), ('k_chunk', ci), ('colsum_out', vp), ('tile', ci), ('drop_thresh', cu32),
                ('drop_scale', cf), ('vec_epi', ci), ('slab', vp), ('slab_floats', cl), ('slab_mode', ci), ('pre_add', vp), ('ldpre', ci), ('gate_bwd', ci), ('B3', vp), ('b3_stride', cl), ('ldb3', ci)]


GemmTile = collections.namedtuple('GemmTile', 'rows cols bk stages occ suffix kernels')
NNR_ERR_ARG, NNR_ERR_UNSUPPORTED = -1, -3


class LstmProblem(C.Structure):
    _fields_ = [('bs', vp), ('off', vp), ('slen', vp), ('prev_f', vp), ('prev_r', vp), ('n', ci), ('L', ci), ('gates', vp),
                ('cell', vp), ('hout', vp), ('cn', vp), ('wf', vp), ('wb', vp), ('dh', vp), ('dcn', vp), ('sync', vp)]


class TransposeDesc(C.Structure):
    _fields_ = [('inp', vp), ('out', vp), ('rows', ci), ('cols', ci)]


class CorpusTables(C.Structure):
    _fields_ = [(k, vp) for k in ('news_category', 'news_subCategory', 'title_text', 'title_mask', 'title_entity', 'abstract_text',
                                  'abstract_mask', 'abstract_entity', 'beh_user', 'beh_history', 'beh_history_mask', 'beh_line',
                                  'graph_table', 'cmask_table', 'cidx_table')] + [(k, ci) for k in ('T', 'C', 'H', 'G', 'K1')]


class BatchOut(C.Structure):
    _fields_ = [(k, vp) for k in ('user_id', 'u_cat', 'u_sub', 'u_tt', 'u_tm', 'u_te', 'u_ct', 'u_cm', 'u_ce', 'u_hmask', 'u_graph',
                                  'u_cmask', 'u_cidx', 'n_cat', 'n_sub', 'n_tt', 'n_tm', 'n_te', 'n_ct', 'n_cm', 'n_ce')]


class PoolArgs(C.Structure):
    _fields_ = [('x', vp), ('ldx', ci), ('D', ci), ('n', ci), ('L', ci), ('packed', ci), ('off', vp), ('slen', vp),
                ('order', vp), ('mask', vp), ('mask_div', ci), ('score', vp), ('v', vp), ('ldv', ci), ('scale', cf),
                ('alpha', vp), ('out', vp), ('ldo', ci), ('add_in', vp), ('ldadd', ci), ('dout', vp), ('lddo', ci),
                ('dout2', vp), ('lddo2', ci), ('dx', vp), ('lddx', ci), ('dx_accumulate', ci), ('dscore', vp), ('dv', vp),
                ('lddv', ci), ('th', vp), ('ldth', ci), ('A', ci), ('w2', vp),
                ('alpha_b', vp), ('dout_b', vp), ('lddo_b', ci), ('dscore_b', vp), ('v_b', vp), ('ldv_b', ci), ('scale_b', cf)]


# The C-ABI, stated once: entry point -> 'return kind, then the kind of every parameter in header order' (tests/test_cabi_exports.py
# compares every word with include/nnr_hip.h).  lib() derives argtypes / restype from it, so call sites pass plain Python values, and the
# tape (nnr_amd/tape.py) encodes a recorded call by these kinds.  i32 int | i64 long, int64_t | u64 size_t, uint64_t | f32 float |
# seed uint32_t (every scalar one is a dropout seed, but the sampler's run seed: tape.RUN_SEED_ARGS) | ptr data pointer | handle nnr_tape*, nnr_dp_ctx* (opaque host objects, also as **
# out-parameters) | cstr char* | stream hipStream_t | a mirror class's name: pointer to that struct.
SIGNATURES = {
    'nnr_version': 'i32',
    'nnr_gemm_f32': 'i32 GemmArgs stream',
    'nnr_gemm_tile_for': 'i32 GemmArgs',
    'nnr_gemm_tile_info': 'i32 i32 i32 i32 ptr cstr cstr i32',
    'nnr_split_bf16x3': 'i32 ptr i32 i32 i32 i32 ptr i64 stream',
    'nnr_seq_plan': 'i32 ptr ptr i32 i32 ptr ptr ptr ptr ptr ptr ptr ptr ptr ptr ptr stream',
    'nnr_seq_plan_pair': 'i32 ptr ptr i32 ptr ptr i32 i32 ptr ptr ptr ptr ptr ptr ptr ptr ptr ptr ptr stream',
    'nnr_cne_pair_map': 'i32 ptr ptr i32 i32 ptr ptr ptr stream',
    'nnr_mask_cover': 'i32 ptr i32 i32 ptr stream',
    'nnr_seq_rowmap': 'i32 ptr ptr ptr i32 i32 ptr stream',
    'nnr_lstm_dims': 'i32 i32 ptr ptr ptr',
    'nnr_lstm_pack_weights': 'i32 ptr ptr ptr ptr ptr ptr ptr ptr i32 i32 ptr ptr ptr ptr ptr stream',
    'nnr_lstm_unpack_grads': 'i32 ptr ptr ptr i32 i32 ptr ptr ptr ptr ptr ptr ptr ptr i32 i32 stream',
    'nnr_lstm_sync_bytes': 'u64 i32',
    'nnr_lstm_sync_diag_offset': 'u64 i32',
    'nnr_lstm_set_timeout_counter': 'i32 ptr',
    'nnr_lstm_fwd': 'i32 LstmProblem i32 i32 stream',
    'nnr_lstm_bwd': 'i32 LstmProblem i32 i32 stream',
    'nnr_gru_dims': 'i32 i32 i32 ptr ptr ptr',
    'nnr_gru_pack_weights': 'i32 ptr ptr ptr ptr i32 i32 ptr ptr ptr ptr stream',
    'nnr_gru_unpack_grads': 'i32 ptr ptr ptr i32 i32 ptr ptr ptr ptr stream',
    'nnr_gru_fwd': 'i32 ptr ptr ptr ptr i32 i32 i32 ptr ptr ptr ptr stream',
    'nnr_gru_bwd': 'i32 ptr ptr ptr ptr ptr i32 i32 i32 ptr stream',
    'nnr_gru_zero_empty': 'i32 ptr ptr i32 i32 stream',
    'nnr_gru_tanh_bwd': 'i32 ptr ptr ptr i32 i32 ptr stream',
    'nnr_attn_pool_fwd': 'i32 PoolArgs stream',
    'nnr_attn_pool_bwd': 'i32 PoolArgs stream',
    'nnr_gate_bwd': 'i32 ptr ptr ptr ptr ptr ptr i32 i32 stream',
    'nnr_packed_seq_sum': 'i32 ptr i32 ptr ptr i32 ptr stream',
    'nnr_slot_workspace_floats': 'i32 i32',
    'nnr_tanh_score_bwd': 'i32 ptr ptr ptr ptr ptr i32 i32 ptr stream',
    'nnr_colsum': 'i32 ptr i32 ptr i32 i32 ptr ptr stream',
    'nnr_rowdot': 'i32 ptr i32 ptr ptr i32 i32 ptr stream',
    'nnr_small_embed_fwd': 'i32 ptr ptr i32 i32 ptr i32 f32 seed stream',
    'nnr_small_embed_bwd': 'i32 ptr i32 i32 ptr i32 ptr f32 seed stream',
    'nnr_user_rows_fwd': 'i32 ptr i32 ptr i32 i32 ptr f32 seed stream',
    'nnr_user_rows_bwd': 'i32 ptr ptr i32 i32 i32 ptr f32 seed stream',
    'nnr_embed_gather': 'i32 ptr ptr i64 ptr i32 ptr f32 seed stream',
    'nnr_embed_scatter': 'i32 ptr ptr i64 i32 ptr f32 seed stream',
    'nnr_embed_scatter_dyn': 'i32 ptr ptr i64 ptr i32 ptr f32 seed stream',
    'nnr_token_sort_workspace_bytes': 'u64 i64 i32',
    'nnr_token_sort': 'i32 ptr i64 ptr i32 ptr ptr ptr ptr ptr u64 stream',
    'nnr_embed_scatter_sorted_workspace_floats': 'u64 i64',
    'nnr_embed_scatter_sorted': 'i32 ptr ptr ptr i64 i32 i32 ptr f32 seed ptr stream',
    'nnr_transpose2d': 'i32 ptr ptr i64 i32 i32 stream',
    'nnr_transpose_batch': 'i32 TransposeDesc i32 stream',
    'nnr_permute': 'i32 ptr ptr i32 i32 i32 i32 i64 i64 i64 i64 i64 i64 i64 i64 i32 stream',
    'nnr_add': 'i32 ptr ptr i64 f32 stream',
    'nnr_add_atomic': 'i32 ptr ptr i64 f32 stream',
    'nnr_add2d': 'i32 ptr i32 ptr i32 i32 i32 f32 i32 stream',
    'nnr_expand_rows_fwd': 'i32 ptr ptr i32 i32 i32 stream',
    'nnr_expand_rows_bwd': 'i32 ptr ptr i32 i32 i32 stream',
    'nnr_dropout': 'i32 ptr ptr i64 f32 seed stream',
    'nnr_relu_bwd': 'i32 ptr ptr ptr i64 stream',
    'nnr_gcn_aggregate_fwd': 'i32 ptr ptr ptr ptr ptr ptr i32 i32 i32 i32 f32 seed stream',
    'nnr_gcn_aggregate_bwd': 'i32 ptr ptr ptr ptr ptr ptr i32 i32 i32 f32 seed stream',
    'nnr_relu_drop_bwd': 'i32 ptr ptr ptr ptr i64 f32 seed stream',
    'nnr_sigmoid_drop_bwd': 'i32 ptr ptr ptr i64 f32 seed stream',
    'nnr_mhsa_fwd': 'i32 ptr ptr i32 i32 i32 i32 f32 ptr ptr f32 seed stream',
    'nnr_mhsa_bwd': 'i32 ptr ptr ptr ptr i32 i32 i32 i32 f32 ptr f32 seed stream',
    'nnr_mhsa_fwd_packed': 'i32 ptr ptr ptr i32 i32 i32 i32 f32 ptr f32 seed stream',
    'nnr_mhsa_bwd_packed': 'i32 ptr ptr ptr ptr i32 i32 i32 i32 f32 ptr f32 seed stream',
    'nnr_mhsa_pair_map': 'i32 ptr ptr ptr ptr i32 i32 ptr ptr stream',
    'nnr_mhsa_fwd_paired': 'i32 ptr ptr ptr ptr i32 i32 i32 f32 ptr f32 seed stream',
    'nnr_mhsa_bwd_paired': 'i32 ptr ptr ptr ptr ptr i32 i32 i32 f32 ptr f32 seed stream',
    'nnr_sue_x0_fwd': 'i32 ptr ptr ptr i32 i32 i32 i32 f32 seed ptr stream',
    'nnr_sue_x0_bwd': 'i32 ptr ptr ptr ptr i32 i32 i32 i32 f32 seed stream',
    'nnr_sue_slice_fwd': 'i32 ptr ptr ptr i32 i32 i32 i32 stream',
    'nnr_sue_slice_bwd': 'i32 ptr ptr i32 i32 i32 i32 stream',
    'nnr_sue_intra_fwd': 'i32 ptr ptr ptr ptr i32 i32 i32 i32 i32 i32 ptr ptr stream',
    'nnr_sue_intra_bwd': 'i32 ptr ptr ptr ptr ptr ptr i32 i32 i32 i32 i32 i32 ptr ptr ptr ptr stream',
    'nnr_sue_seg_pool_fwd': 'i32 ptr ptr ptr i32 i32 i32 i32 i32 f32 ptr ptr stream',
    'nnr_sue_seg_pool_bwd': 'i32 ptr ptr ptr ptr ptr i32 i32 i32 i32 i32 f32 ptr ptr ptr stream',
    'nnr_cand_attn_ws_floats': 'i32 i32 i32 i32 i32',
    'nnr_cand_attn_fwd': 'i32 ptr ptr ptr ptr i32 ptr i32 i32 i32 i32 i32 i32 ptr ptr stream',
    'nnr_cand_attn_bwd': 'i32 ptr ptr ptr ptr i32 ptr ptr ptr i32 i32 i32 i32 i32 i32 ptr ptr ptr i32 ptr ptr stream',
    'nnr_pers_attn_ws_floats': 'i32 i32 i32 i32',
    'nnr_pers_attn_fwd': 'i32 ptr ptr ptr i32 ptr ptr i32 ptr i32 i32 i32 i32 ptr ptr stream',
    'nnr_pers_attn_bwd': 'i32 ptr ptr ptr i32 ptr ptr i32 ptr ptr ptr i32 i32 i32 i32 ptr ptr ptr ptr ptr stream',
    'nnr_omap_ws_floats': 'i32 i32 i32 i32 i32 i32',
    'nnr_omap_fwd': 'i32 ptr i32 ptr ptr ptr i32 i32 i32 i32 i32 ptr ptr ptr ptr ptr ptr ptr stream',
    'nnr_omap_bwd': 'i32 ptr i32 ptr ptr ptr ptr ptr ptr ptr ptr ptr i32 i32 i32 i32 i32 ptr i32 ptr ptr ptr stream',
    'nnr_omap_reg_fwd': 'i32 ptr i32 i32 f32 ptr ptr stream',
    'nnr_omap_reg_bwd': 'i32 ptr ptr ptr i32 i32 f32 ptr stream',
    'nnr_bag_mean_fwd': 'i32 ptr i32 i32 ptr ptr i32 ptr ptr i32 i32 i32 i32 ptr i32 i32 i32 ptr ptr stream',
    'nnr_bag_mean_bwd_ws_floats': 'u64 i64',
    'nnr_bag_mean_bwd': 'i32 ptr i32 ptr i32 i32 i32 ptr ptr ptr i64 i32 i32 i32 i32 i32 i32 i32 ptr ptr stream',
    'nnr_row_dist_fwd': 'i32 ptr i32 ptr i32 i32 i32 f32 ptr ptr stream',
    'nnr_row_dist_bwd': 'i32 ptr i32 ptr i32 ptr ptr i32 i32 f32 ptr i32 ptr i32 stream',
    'nnr_kcnn_image_fwd': 'i32 ptr i32 ptr ptr ptr i32 i32 i32 i32 ptr stream',
    'nnr_kcnn_image_bwd': 'i32 ptr ptr i32 i32 i32 i32 ptr ptr ptr stream',
    'nnr_window_max_fwd': 'i32 ptr i32 ptr i32 i32 i32 i32 ptr ptr stream',
    'nnr_window_max_bwd_ws_floats': 'u64 i32 i32',
    'nnr_window_max_bwd': 'i32 ptr ptr i32 i32 i32 i32 i32 ptr ptr ptr stream',
    'nnr_view_pool_fwd': 'i32 ptr ptr ptr ptr i32 ptr ptr ptr i32 ptr ptr ptr i32 i32 i32 ptr ptr stream',
    'nnr_view_pool_bwd': 'i32 ptr ptr ptr i32 ptr ptr i32 ptr ptr i32 ptr i32 i32 ptr ptr ptr ptr ptr ptr ptr ptr ptr stream',
    'nnr_conv1d_image_fwd': 'i32 ptr i32 ptr i32 i32 i32 i32 f32 seed ptr stream',
    'nnr_conv1d_dz_pad': 'i32 ptr ptr i32 i32 i32 i32 ptr stream',
    'nnr_conv1d_image_bwd': 'i32 ptr i32 i32 i32 i32 f32 seed ptr stream',
    'nnr_hdc_seq_fwd': 'i32 ptr i32 ptr i32 ptr i32 ptr ptr ptr i32 i32 i32 i32 ptr ptr ptr ptr ptr stream',
    'nnr_hdc_ln_relu_fwd': 'i32 ptr i32 ptr ptr i32 i32 i32 f32 ptr ptr i32 ptr stream',
    'nnr_hdc_ln_bwd_ws_floats': 'u64 i32 i32 i32',
    'nnr_hdc_ln_relu_bwd': 'i32 ptr ptr ptr i32 ptr ptr i32 i32 i32 ptr ptr ptr stream',
    'nnr_hdc_unpad_add': 'i32 ptr ptr i32 i32 i32 i32 ptr stream',
    'nnr_conv3d_pool_dims': 'i32 i32 i32 i32 i32 i32 i32 i32 i32 ptr ptr ptr',
    'nnr_conv3d_pool_fwd': 'i32 ptr i64 i64 i64 i64 i64 ptr ptr i32 i32 i32 i32 i32 i32 i32 i32 i32 i32 ptr ptr stream',
    'nnr_conv3d_pool_bwd_ws_floats': 'u64 i32 i32 i32 i32 i32 i32 i32 i32 i32',
    'nnr_conv3d_pool_bwd': 'i32 ptr ptr ptr ptr i64 i64 i64 i64 i64 ptr i32 i32 i32 i32 i32 i32 i32 i32 i32 i32 ptr ptr ptr ptr stream',
    'nnr_corpus_batch': 'i32 CorpusTables BatchOut ptr ptr i32 i32 i32 stream',
    'nnr_history_graph': 'i32 ptr ptr i32 i32 i32 i32 ptr ptr ptr stream',
    'nnr_negative_sample': 'i32 ptr ptr ptr ptr i32 i32 seed i32 ptr i32 stream',
    'nnr_list_scores': 'i32 ptr i64 i32 ptr i64 i32 ptr ptr i64 i32 ptr stream',
    'nnr_cne_pair_triples': 'i32 ptr ptr ptr ptr i64 i32 i32 i32 i64 i64 ptr ptr ptr ptr ptr stream',
    'nnr_rank_metrics': 'i32 ptr ptr ptr i32 ptr ptr stream',
    'nnr_topk_workspace_bytes': 'u64 i64 i64 i32',
    'nnr_topk_scores': 'i32 ptr i64 i32 ptr i64 i32 i32 ptr ptr i32 i32 i32 ptr ptr ptr i64 stream',
    'nnr_pool_rank_workspace_bytes': 'u64 i64 i64 i64',
    'nnr_pool_ranks': 'i32 ptr i64 i32 ptr i64 i32 i32 ptr ptr i32 i32 ptr ptr i64 ptr ptr ptr ptr i64 stream',
    'nnr_topk_archive_scores': 'i32 ptr i64 i32 i32 i32 f32 ptr i64 i32 i32 ptr ptr i32 i32 i32 ptr ptr ptr i64 stream',
    'nnr_pool_archive_ranks': 'i32 ptr i64 i32 i32 i32 f32 ptr i64 i32 i32 ptr ptr i32 i32 ptr ptr i64 ptr ptr ptr ptr i64 stream',
    'nnr_logits_loss_fwd': 'i32 ptr ptr i32 i32 i32 ptr ptr ptr stream',
    'nnr_logits_fwd': 'i32 ptr ptr i32 i32 i32 ptr stream',
    'nnr_nls_loss': 'i32 ptr i32 i32 ptr ptr stream',
    'nnr_logits_bwd': 'i32 ptr ptr ptr i32 i32 i32 ptr ptr i32 stream',
    'nnr_layernorm_fwd': 'i32 ptr ptr ptr f32 i64 i32 ptr ptr ptr ptr ptr f32 seed stream',
    'nnr_layernorm_bwd': 'i32 ptr ptr ptr ptr i64 i32 ptr ptr ptr stream',
    'nnr_sumsq': 'i32 ptr i64 ptr stream',
    'nnr_sumsq_part': 'i32 ptr i64 ptr ptr i32 stream',
    'nnr_clip_adam': 'i32 ptr ptr ptr ptr i64 ptr f32 f32 f32 f32 f32 f32 f32 i32 stream',
    'nnr_adam_skipped_steps': 'i32 ptr i32',
    'nnr_adam_skipped_peek': 'i32 ptr',
    'nnr_dp_unique_id': 'i32 ptr',
    'nnr_dp_init': 'i32 ptr i32 i32 handle',
    'nnr_dp_allreduce': 'i32 handle ptr u64 stream',
    'nnr_dp_broadcast': 'i32 handle ptr u64 i32 stream',
    'nnr_dp_destroy': 'i32 handle',
    'nnr_dp_emulate_ranks': 'i32 handle i32',
    'nnr_dp_busy': 'i32 ptr i64 i32 i32 stream',
    'nnr_rows_touch': 'i32 ptr i64 ptr i32 ptr stream',
    'nnr_rows_compact': 'i32 ptr i32 ptr ptr stream',
    'nnr_rows_pack': 'i32 ptr ptr i32 i32 ptr stream',
    'nnr_rows_unpack': 'i32 ptr ptr i32 i32 ptr stream',
    'nnr_fusion_rows_fwd': 'i32 ptr ptr ptr ptr i32 ptr ptr i32 i32 i32 ptr i32 f32 seed seed stream',
    'nnr_fusion_rows_bwd': 'i32 ptr ptr i32 ptr ptr i32 i32 i32 ptr i32 ptr ptr f32 seed seed stream',
    'nnr_fusion_rows_bwd_det': 'i32 ptr ptr i32 ptr ptr i32 i32 i32 i32 i32 ptr i32 ptr ptr f32 seed seed stream',
    'nnr_click_loss': 'i32 ptr ptr i32 i32 i32 ptr ptr ptr ptr ptr ptr stream',
    'nnr_wbag_dims': 'i32 i32 i32 i32 ptr ptr ptr',
    'nnr_wbag_fwd_ws_floats': 'u64 i32 i32 i32 i32 i32',
    'nnr_wbag_fwd': 'i32 ptr i32 i32 ptr ptr ptr i32 i32 i32 ptr ptr ptr i32 i32 i32 f32 seed seed ptr ptr ptr stream',
    'nnr_wbag_bwd_ws_floats': 'u64 i64 i32',
    'nnr_wbag_bwd': 'i32 ptr ptr ptr i64 ptr ptr i32 i32 i32 ptr ptr i32 i32 i32 i32 i32 f32 seed seed ptr ptr stream',
    'nnr_cosine_loss': 'i32 ptr ptr i32 i32 i32 ptr ptr ptr ptr ptr ptr stream',
    'nnr_tanh_drop_bwd': 'i32 ptr ptr ptr i64 f32 seed stream',
    'nnr_fill_zero': 'i32 ptr u64 stream',
    'nnr_copy_bytes': 'i32 ptr ptr u64 stream',
    'nnr_fill_column_u8': 'i32 ptr i32 i32 i32 i32 stream',
    'nnr_tape_create': 'i32 handle',
    'nnr_tape_destroy': 'i32 handle',
    'nnr_tape_fn_id': 'i32 cstr',
    'nnr_tape_fn_nargs': 'i32 i32',
    'nnr_tape_call': 'i32 handle i32 stream ptr i32 ptr ptr ptr i32 i32 ptr ptr',
    'nnr_tape_wait_stream': 'i32 handle stream stream',
    'nnr_tape_event_record': 'i32 handle u64 stream',
    'nnr_tape_event_wait': 'i32 handle stream u64',
    'nnr_tape_segment': 'i32 handle',
    'nnr_tape_patch': 'i32 handle u64 i32 i32 i64',
    'nnr_tape_finalize': 'i32 handle',
    'nnr_tape_prepare_timing': 'i32 handle i32',
    'nnr_tape_info': 'i32 handle ptr ptr ptr ptr ptr',
    'nnr_tape_replay': 'i32 handle i32 ptr i32 ptr i32 i32',
    'nnr_tape_timings': 'i32 handle i32 ptr i32',
    'nnr_tape_timeline': 'i32 handle i32 ptr ptr ptr i32',
    'nnr_tape_last_error': 'i32 handle ptr ptr cstr i32',
}
SYMBOLS = list(SIGNATURES)
STRUCTS = {'nnr_gemm_args': GemmArgs, 'nnr_lstm_problem': LstmProblem, 'nnr_pool_args': PoolArgs, 'nnr_transpose_desc': TransposeDesc,
           'nnr_corpus_tables': CorpusTables, 'nnr_batch_out': BatchOut}
DEVICE_STRUCTS = {'TransposeDesc'}     # descriptor tables that live in DEVICE memory: passed (and recorded) like any data pointer
_CTYPES = {'i32': ci, 'i64': cl, 'u64': C.c_size_t, 'f32': cf, 'seed': cu32, 'ptr': vp, 'handle': vp, 'cstr': C.c_char_p, 'stream': vp}
_CTYPES.update((c.__name__, vp if c.__name__ in DEVICE_STRUCTS else C.POINTER(c)) for c in STRUCTS.values())


def kinds(name):
    """Parameter kinds of an entry point, in header order (the return kind is SIGNATURES[name].split()[0])."""
    return SIGNATURES[name].split()[1:]


class NnrHipError(RuntimeError):
    pass


def build(force=False):
    """Compile libnnr_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        bdir = os.path.join(_HERE, 'csrc', 'build')
        if os.path.isdir(bdir):
            for f in os.listdir(bdir):
                os.remove(os.path.join(bdir, f))
    subprocess.check_call(['bash', os.path.join(_HERE, 'csrc', 'build.sh')])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NnrHipError('libnnr_hip.so not found at %s -- run `python -c "import __graft_entry__ as g; g.build()"` '
                              '(there is no CPU / PyTorch fallback on the product path)' % LIB_PATH)
        # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so); it must be in the process BEFORE this library is
        # loaded, so that the library's DT_NEEDED entry binds to that copy.  Loaded first, libnnr_hip.so would pull in /opt/rocm's
        # runtime next to torch's: two HIP runtimes in one process, and every torch stream / allocation handed to an entry point is
        # foreign to the second one (each call fails with NNR_ERR_LAUNCH) -- found by running build() and smoke() in ONE process.
        import torch  # noqa: F401
        _lib = C.CDLL(LIB_PATH)
        for name, sig in SIGNATURES.items():
            ret, *params = [_CTYPES[k] for k in sig.split()]
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = ret, params
    return _lib


_tiles = None


def gemm_tiles():
    """csrc/gemm.hip's tile table, read once: {tile id: GemmTile}.  `kernels` maps each operand layout the row has kernels for ('nt', 'nn',
    'tn') to the instantiation as rocprofv3 prints it ('' for the skinny tile); the live profile's family is 'gemm_<layout>_<suffix>'."""
    global _tiles
    if _tiles is None:
        tiles, dims, suffix, kernel = {}, (ci * 6)(), C.create_string_buffer(64), C.create_string_buffer(64)
        for index in itertools.count():
            kernels = {}
            for lay, ta, tb in (('nt', 0, 0), ('nn', 0, 1), ('tn', 1, 1)):
                rc = lib().nnr_gemm_tile_info(index, ta, tb, dims, suffix, kernel, 64)
                if rc == 0:
                    kernels[lay] = kernel.value.decode()
                elif rc != NNR_ERR_UNSUPPORTED:
                    break
            else:
                tiles[dims[0]] = GemmTile(*dims[1:], suffix.value.decode(), kernels)
                continue
            break                           # NNR_ERR_ARG: past the last row
        _tiles = tiles
    return _tiles


def build_id():
    """Identity of the kernels that are running: sha256 over the sources libnnr_hip.so is built from (csrc/*.hip, common.h, the
    header) and, separately, over the loaded binary.  profiles/pmc_traffic.json carries both: counter traffic collected on another
    build is not quoted (nnr_amd.profile.pmc_traffic)."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(_HERE, 'csrc')
    for f in sorted(os.listdir(src)):
        if f.endswith(('.hip', '.h')):
            h.update(f.encode())
            h.update(open(os.path.join(src, f), 'rb').read())
    h.update(open(os.path.join(os.path.dirname(_HERE), 'include', 'nnr_hip.h'), 'rb').read())
    lib_hash = hashlib.sha256(open(LIB_PATH, 'rb').read()).hexdigest()[:16] if os.path.exists(LIB_PATH) else None
    return {'src_sha256': h.hexdigest()[:16], 'lib_sha256': lib_hash}


CALLS = [0]          # C-ABI calls checked so far (bench.py reports calls per step; each is one or a few kernel launches)


def check(rc, what, unsupported=None, counted=True):
    """unsupported: the sentence to raise with when the entry point answers NNR_ERR_UNSUPPORTED (sizes beyond a kernel family's limits).
    counted=False: a size query that launches nothing and is not one of a step's calls."""
    CALLS[0] += counted
    if rc == NNR_ERR_UNSUPPORTED and unsupported is not None:
        raise NnrHipError('%s: %s' % (what, unsupported))
    if rc != 0:
        raise NnrHipError('%s failed with code %d' % (what, rc))
