"""ctypes binding of libpairec_gpu.so (include/pairec_gpu.h).

The library is the product: there is no CPU fallback.  Importing this module without the built
extension, or calling it without a gfx950 GPU, fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpairec_gpu.so")

# every symbol include/pairec_gpu.h declares (tests/test_abi.py checks the two stay in sync)
EXPORTS = [
    "pg_last_error", "pg_version", "pg_device_count", "pg_init", "pg_shutdown", "pg_synchronize", "pg_device_malloc",
    "pg_device_free", "pg_memcpy_h2d", "pg_memcpy_d2h", "pg_table_create", "pg_table_destroy",
    "pg_table_fill_synthetic", "pg_table_upload", "pg_table_download", "pg_table_swap",
    "pg_table_info", "pg_table_gather", "pg_recall_topk", "pg_recall_topk_dev", "pg_recall_topk_l2", "pg_recall_topk_l2_dev", "pg_recall_topk_where", "pg_table_view_create",
    "pg_topk_merge_dev", "pg_model_load", "pg_model_destroy", "pg_model_num_outputs", "pg_model_f16_stats", "pg_rank_dnn3", "pg_rank_dnn3_dev",
    "pg_rank_fm2t", "pg_rank_fm2t_dev", "pg_expr_compile", "pg_expr_free", "pg_expr_num_vars", "pg_expr_set_score_rewrites", "pg_expr_compile_typed", "pg_expr_is_antlr", "pg_fuse_scores_dev",
    "pg_expr_var_name", "pg_expr_eval", "pg_expr_eval_dev", "pg_sort_scores", "pg_sort_scores_dev",
    "pg_dpp", "pg_stats", "pg_last_scan_kernel_ms", "pg_rows_to_local_dev", "pg_widen_f32_dev",
    "pg_hbm_read_probe", "pg_table_screen_info", "pg_table_derived_info", "pg_table_derived_read", "pg_ssd", "pg_ssd_emb", "pg_features_create", "pg_features_destroy", "pg_features_set_column",
    "pg_features_column_index", "pg_features_num_columns", "pg_features_gather_i32_dev",
    "pg_features_gather_f32_dev", "pg_rank_fm2t_rows_dev", "pg_rank_fm2t_rows", "pg_recommend_dnn3_dev", "pg_set_option",
    "pg_table_fill_gaussian", "pg_table_fill_mixture", "pg_group_exchange_stats", "pg_dpp_ex", "pg_i2i_recall", "pg_online_vector_recall", "pg_fm2t_user_embedding",
    "pg_fm2t_user_embedding_dev", "pg_recommend_dnn3_begin", "pg_recommend_end",
    "pg_coalescer_create", "pg_coalescer_destroy", "pg_coalescer_recall", "pg_coalescer_rank_dnn3",
    "pg_coalescer_recommend", "pg_coalescer_stats", "pg_coalescer_create_scene", "pg_coalescer_i2i_recall", "pg_coalescer_recall_l2",
    "pg_coalescer_online_recall", "pg_coalescer_rank", "pg_coalescer_rank_fm2t", "pg_coalescer_recommend_ex",
    "pg_coalescer_dpp", "pg_coalescer_ssd", "pg_recommend_end_timed", "pg_debug_stall",
    "pg_fm2t_item_rows_build", "pg_fm2t_item_rows_update", "pg_fm2t_item_rows_destroy", "pg_rank_fm2t_irows_dev",
    "pg_rank_fm2t_irows",
    "pg_topk_merge_lists_dev", "pg_owned_compact_dev", "pg_scatter_f32_dev", "pg_dpp_candidates_dev",
    "pg_gather_owned_rows_dev", "pg_dpp_batch_dev", "pg_dpp_kernel_matrix_dev", "pg_features_eval_dev",
    "pg_group_create", "pg_group_destroy", "pg_group_size", "pg_group_ctx", "pg_group_table", "pg_group_table_create",
    "pg_group_table_fill_synthetic", "pg_group_table_upload", "pg_group_model_load", "pg_group_recommend",
    "pg_group_recommend_begin", "pg_group_recommend_end", "pg_group_info", "pg_coalescer_create_group",
    "pg_router_create", "pg_router_destroy", "pg_router_recommend", "pg_router_recall", "pg_router_stats",
    "pg_index_build", "pg_index_destroy", "pg_index_recall_topk", "pg_index_recall_topk_dev", "pg_index_recall_topk_l2",
    "pg_index_recall_topk_l2_dev", "pg_index_stats", "pg_index_attach", "pg_index_detach", "pg_index_serving_stats",
    "pg_index_read", "pg_index_bounds", "pg_index_recall_topk_where", "pg_index_where_read", "pg_index_where_stats",
    "pg_index_refresh", "pg_index_refresh_stats", "pg_index_screen_probe",
    "pg_where_compile", "pg_where_free", "pg_where_num_columns", "pg_where_column_name", "pg_where_eval_host",
    "pg_recall_topk_where_ex", "pg_index_recall_topk_where_ex", "pg_table_view_create_ex", "pg_where_bits", "pg_where_stats",
    "pg_exclude_compact_dev", "pg_recall_topk_exclude", "pg_recall_topk_exclude_dev", "pg_i2i_recall_exclude",
    "pg_coalescer_recall_exclude",
    "pg_simtable_create", "pg_simtable_upload", "pg_simtable_info", "pg_simtable_destroy", "pg_cf_recall", "pg_cf_recall_dev",
    "pg_rtu2i_compile", "pg_rtu2i_free", "pg_rtu2i_trigger_count", "pg_rtu2i_triggers_host", "pg_rtu2i_triggers", "pg_rtu2i_triggers_dev",
    "pg_rtu2i_expand", "pg_rtu2i_expand_dev", "pg_rtu2i_recall", "pg_rtu2i_recall_dev",
    "pg_fanin_merge_dev", "pg_recommend_candidates_dnn3_dev",
    "pg_trim_out_cap", "pg_candidates_trim_dev", "pg_recommend_cascade_dnn3_dev",
    "pg_blend_out_cap", "pg_candidates_blend_dev", "pg_candidates_blend_host",
    "pg_trim2_out_cap", "pg_candidates_trim2_dev", "pg_candidates_trim2_host",
    "pg_diversity_rules_host", "pg_diversity_rules_dev", "pg_diversity_rules_features_dev", "pg_diversity_rules",
    "pg_expr_compile_govaluate", "pg_expr_eval_host",
    "pg_cond_compile", "pg_cond_free", "pg_cond_num_rules", "pg_cond_num_user_slots", "pg_cond_user_slot_name",
    "pg_cond_user_slot_is_float", "pg_cond_match_host", "pg_boost_scores_host", "pg_item_state_filter_dev", "pg_boost_scores_dev",
    "pg_item_state_filter", "pg_boost_scores",
    "pg_distinct_ids_host", "pg_distinct_ids_dev", "pg_distinct_ids",
    "pg_candidates_dimcap_host", "pg_candidates_dimcap_dev", "pg_candidates_dimcap",
    "pg_classcut_compile", "pg_classcut_free", "pg_classcut_num_classes", "pg_classcut_reads_recall_name", "pg_classcut_out_cap",
    "pg_classcut_masks_host", "pg_candidates_classcut_host", "pg_classcut_masks_dev", "pg_candidates_classcut_dev",
    "pg_candidates_classcut",
    "pg_mix_compile", "pg_mix_free", "pg_mix_num_strategies", "pg_mix_num_user_slots", "pg_mix_user_slot_name", "pg_mix_user_slot_is_float",
    "pg_mix_sort_host", "pg_mix_sort_dev", "pg_mix_sort", "pg_ssd_sort_dev",
    "pg_traffic_compile", "pg_traffic_free", "pg_traffic_num_targets", "pg_traffic_table", "pg_traffic_sort_host", "pg_traffic_sort_dev",
    "pg_traffic_sort",
    "pg_cold_create", "pg_cold_free", "pg_cold_recall_host", "pg_cold_recall_dev", "pg_cold_recall", "pg_cold_stats",
    "pg_xtable_create", "pg_xtable_upload_item2x", "pg_xtable_upload_x2item", "pg_xtable_info", "pg_xtable_destroy",
    "pg_x2i_recall", "pg_x2i_recall_dev", "pg_x2i_recall_host", "pg_rtu2i_x_recall", "pg_rtu2i_x_recall_dev",
    "pg_bloom_estimate", "pg_bloom_murmur3_host", "pg_bloom_keys_create", "pg_bloom_keys_create_decimal", "pg_bloom_keys_free",
    "pg_bloom_create", "pg_bloom_free", "pg_bloom_info", "pg_bloom_slot_write", "pg_bloom_slot_read", "pg_bloom_slot_clear",
    "pg_bloom_exists_dev", "pg_bloom_filter_dev", "pg_bloom_add_dev", "pg_bloom_exists", "pg_bloom_filter", "pg_bloom_add",
    "pg_bloom_exists_host", "pg_bloom_add_host", "pg_bloom_filter_host", "pg_bloom_slot_write_host",
    "pg_hottable_create", "pg_hottable_upload", "pg_hottable_info", "pg_hottable_destroy",
    "pg_hot_recall_dev", "pg_hot_recall", "pg_hot_recall_host",
]


class PgStats(C.Structure):
    _fields_ = [("recall_calls", C.c_uint64), ("recall_rows_scanned", C.c_uint64),
                ("recall_rescans", C.c_uint64), ("rank_calls", C.c_uint64),
                ("rank_items", C.c_uint64), ("sort_calls", C.c_uint64), ("sort_items", C.c_uint64),
                ("last_recall_ms", C.c_double), ("last_rank_ms", C.c_double),
                ("last_sort_ms", C.c_double), ("recall_predicted", C.c_uint64),
                ("recall_suspects", C.c_uint64), ("recall_suspect_queries", C.c_uint64), ("recall_i4m_pairs", C.c_uint64),
                ("recall_screen_overflows", C.c_uint64), ("recall_record_growths", C.c_uint64),
                ("recall_rescored", C.c_uint64), ("sort_split_calls", C.c_uint64),
                ("ssd_grid_calls", C.c_uint64), ("ssd_reg_calls", C.c_uint64), ("ssd_generic_calls", C.c_uint64),
                ("dpp_wave8_calls", C.c_uint64), ("dpp_wave16_calls", C.c_uint64), ("dpp_block_calls", C.c_uint64),
                ("rank_ws_calls", C.c_uint64), ("rank_rs_calls", C.c_uint64), ("rank_ls_calls", C.c_uint64),
                ("rank_x3_calls", C.c_uint64), ("rank_h2_calls", C.c_uint64), ("rank_isw_calls", C.c_uint64),
                ("rank_mlp_calls", C.c_uint64)]


class PgWhereStats(C.Structure):
    _fields_ = [("builds", C.c_uint64), ("hits", C.c_uint64), ("last_build_ms", C.c_double), ("bytes", C.c_uint64),
                ("epoch", C.c_uint64), ("admitted", C.c_uint64)]


class PgColdStats(C.Structure):
    _fields_ = [("prefix_builds", C.c_uint64), ("prefix_hits", C.c_uint64), ("bytes", C.c_uint64), ("epoch", C.c_uint64),
                ("admitted", C.c_uint64)]


class PgIndexParams(C.Structure):
    _fields_ = [("n_lists", C.c_uint32), ("train_rows", C.c_uint32), ("iters", C.c_uint32), ("seed", C.c_uint64)]


class PgIndexStats(C.Structure):
    _fields_ = [("n_lists", C.c_uint32), ("dim", C.c_uint32), ("rows", C.c_uint64), ("generation", C.c_uint64),
                ("max_radius", C.c_float), ("mean_radius", C.c_float), ("largest_list", C.c_uint32), ("empty_lists", C.c_uint32),
                ("build_ms", C.c_double), ("calls", C.c_uint64), ("queries", C.c_uint64), ("rows_scored", C.c_uint64),
                ("pairs_scored", C.c_uint64), ("fallback_dense", C.c_uint64), ("fallback_stale", C.c_uint64),
                ("fallback_nonfinite", C.c_uint64), ("fallback_overflow", C.c_uint64),
                ("rows_live", C.c_uint64), ("max_query_scan_rows", C.c_uint64)]


class PgIndexServingStats(C.Structure):
    _fields_ = [("plans", C.c_uint64), ("plans_held", C.c_uint64), ("queries_held", C.c_uint64),
                ("replan_dense", C.c_uint64), ("replan_rounds", C.c_uint64), ("replan_overflow", C.c_uint64),
                ("replan_nonfinite", C.c_uint64), ("skipped_stale", C.c_uint64), ("skipped_switch", C.c_uint64)]


class PgIndexWhereStats(C.Structure):
    _fields_ = [("builds", C.c_uint64), ("hits", C.c_uint64), ("evictions", C.c_uint64), ("entries", C.c_uint64),
                ("bytes", C.c_uint64)]


class PgTableDerived(C.Structure):
    _fields_ = [("elem_bytes", C.c_int32), ("all_finite", C.c_int32), ("max_norm", C.c_float), ("s8", C.c_float),
                ("resid8", C.c_float), ("i4_ok", C.c_int32), ("rho4", C.c_float), ("rmax4", C.c_float), ("lam4", C.c_float),
                ("r2_ok", C.c_int32), ("s8r", C.c_float), ("resid2", C.c_float), ("nx_valid", C.c_int32), ("l2_slack", C.c_float),
                ("pred_model", C.c_int32), ("pred_n_sample", C.c_uint64), ("pred_stride", C.c_uint64)]


# pg_table_derived_info's parts and pg_table_derived_read's arrays (PG_DERIVED_*, PG_DERIVED_ARR_*)
DERIVED_STATS, DERIVED_I4, DERIVED_R2, DERIVED_NX, DERIVED_PRED = 1, 2, 4, 8, 16
DERIVED_ALL = 31
DERIVED_ARRAYS = {"i8": 0, "bf16": 1, "blknorm2": 2, "i4": 3, "i4s": 4, "i8r": 5, "nx": 6, "nxmin": 7, "pred": 8}


class PgRecallExcludeOpts(C.Structure):
    _fields_ = [("metric", C.c_int), ("fs", C.c_void_p), ("where", C.c_void_p)]


class PgCfOpts(C.Structure):
    _fields_ = [("normalize", C.c_int), ("excl_rows", C.c_void_p), ("excl_offsets", C.c_void_p)]


class PgX2iOpts(C.Structure):
    _fields_ = [("normalize", C.c_int), ("max_rule", C.c_int), ("excl_rows", C.c_void_p), ("excl_offsets", C.c_void_p)]


class PgRtU2IConf(C.Structure):
    _fields_ = [("weight_expression", C.c_char_p), ("event_weight", C.c_char_p), ("event_play_time", C.c_char_p),
                ("event_names", C.POINTER(C.c_char_p)), ("n_events", C.c_uint32), ("weight_mode", C.c_char_p),
                ("trigger_count", C.c_uint32), ("limit", C.c_uint32)]


class PgFaninSource(C.Structure):
    _fields_ = [("d_rows", C.c_void_p), ("d_scores", C.c_void_p), ("k", C.c_uint32), ("score_f64", C.c_int)]


class PgTrimRule(C.Structure):
    _fields_ = [("source", C.c_uint8), ("type", C.c_uint8), ("count", C.c_uint32)]


class PgBlendConf(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("retain_num", C.c_uint32), ("n_entries", C.c_uint32), ("source", C.c_uint8 * 8),
                ("weight", C.c_uint32 * 8)]


class PgDivRule(C.Structure):
    _fields_ = [("n_dims", C.c_uint32), ("dims", C.c_uint32 * 4), ("interval", C.c_int32), ("window", C.c_int32),
                ("frequency", C.c_int32), ("weight", C.c_int32)]


class PgDivTerm(C.Structure):
    _fields_ = [("column", C.c_uint32), ("op", C.c_int32), ("value", C.c_longlong)]


class PgDivExclusion(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_uint32)), ("n_positions", C.c_uint32), ("n_terms", C.c_uint32),
                ("terms", PgDivTerm * 4)]


class PgDivConfig(C.Structure):
    _fields_ = [("size", C.c_int32), ("diversity_size", C.c_int32), ("explore_item_size", C.c_int32),
                ("exclude_source_mask", C.c_uint32), ("n_cols", C.c_uint32), ("n_rules", C.c_uint32), ("n_excl", C.c_uint32),
                ("n_multi_value", C.c_uint32), ("rules", PgDivRule * 8), ("excl", PgDivExclusion * 8)]


class PgCondTerm(C.Structure):
    _fields_ = [("name", C.c_char_p), ("domain", C.c_char_p), ("op", C.c_int32), ("type", C.c_int32), ("rhs", C.c_int32),
                ("depth", C.c_uint32), ("bool_and", C.c_uint32), ("n_list", C.c_uint32), ("i", C.c_longlong), ("f", C.c_double),
                ("rhs_name", C.c_char_p), ("list", C.POINTER(C.c_longlong))]


class PgCondRule(C.Structure):
    _fields_ = [("terms", C.POINTER(PgCondTerm)), ("n_terms", C.c_uint32), ("expression", C.c_char_p)]


class PgCondCol(C.Structure):
    _fields_ = [("name", C.c_char_p), ("dtype", C.c_int32)]


class PgDimcapConf(C.Structure):
    _fields_ = [("column", C.c_char_p), ("limit", C.c_uint32), ("null_mode", C.c_uint32), ("has_null", C.c_uint32),
                ("null_value", C.c_int64)]


class PgClasscutRule(C.Structure):
    _fields_ = [("expression", C.c_char_p), ("type", C.c_uint8), ("count", C.c_uint32)]


class PgMixStrategy(C.Structure):
    _fields_ = [("type", C.c_int32), ("positions", C.POINTER(C.c_int32)), ("n_positions", C.c_uint32), ("position_field", C.c_char_p),
                ("number", C.c_int32), ("number_rate", C.c_double), ("source_mask", C.c_uint32), ("terms", C.POINTER(PgCondTerm)),
                ("n_terms", C.c_uint32)]


class PgTrafficTarget(C.Structure):
    _fields_ = [("target_id", C.c_int32), ("control_type", C.c_int32)]


class PgIndexRefreshParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("force", C.c_int)]


class PgIndexRefreshStats(C.Structure):
    _fields_ = [("refreshes", C.c_uint64), ("full", C.c_uint64), ("incremental", C.c_uint64), ("noop", C.c_uint64),
                ("rows_reassigned", C.c_uint64), ("rows_moved", C.c_uint64), ("rows_confirmed_wide", C.c_uint64),
                ("last_generation", C.c_uint64), ("last_ms", C.c_double), ("last_assign_ms", C.c_double)]


class PgDppOptions(C.Structure):
    _fields_ = [("alpha", C.c_double), ("topn", C.c_uint32), ("window", C.c_uint32), ("normalize_emb", C.c_int),
                ("ensure_pos_similarity", C.c_int), ("norm_relevance_score", C.c_int), ("has_table", C.c_int),
                ("hook_dim", C.c_uint32)]


class PgGroupPlan(C.Structure):
    _fields_ = [("k", C.c_uint32), ("dpp_candidates", C.c_uint32), ("dpp_alpha", C.c_double),
                ("dpp_window", C.c_uint32), ("dpp_normalize_emb", C.c_int)]


class PgCoalescerConfig(C.Structure):
    _fields_ = [("k", C.c_uint32), ("max_batch", C.c_uint32), ("max_wait_us", C.c_uint32), ("depth", C.c_uint32),
                ("max_top_n", C.c_uint32), ("max_rank_items", C.c_uint32), ("timeout_us", C.c_uint32)]


class PgRankAlgo(C.Structure):
    _fields_ = [("model", C.c_void_p), ("name", C.c_char_p), ("features", C.c_void_p),
                ("item_field_cols", C.POINTER(C.c_int32)), ("item_rows", C.c_void_p),
                ("output_names", C.POINTER(C.c_char_p))]


class PgSceneConfig(C.Structure):
    _fields_ = [("base", PgCoalescerConfig), ("algos", C.POINTER(PgRankAlgo)), ("n_algos", C.c_uint32),
                ("rank_score", C.c_void_p), ("rerank", C.c_int), ("rerank_candidates", C.c_uint32),
                ("dpp", PgDppOptions), ("query_model", C.c_void_p), ("trigger_table", C.c_void_p),
                ("max_rerank_items", C.c_uint32), ("max_hook_dim", C.c_uint32)]


class PgCoalescerStats(C.Structure):
    # flavours: 0 recall (vector / i2i / online), 1 rank, 2 recommend, 3 dpp
    _fields_ = [("requests", C.c_uint64 * 6), ("batches", C.c_uint64 * 6), ("largest_batch", C.c_uint64 * 6),
                ("replans", C.c_uint64), ("timeouts", C.c_uint64), ("device_ms", C.c_double * 6)]


_lib = None


def load():
    """Load libpairec_gpu.so; raise with build instructions if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "pairec_amd: %s not found — build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_size_t
    P = C.POINTER
    L.pg_last_error.restype = C.c_char_p
    L.pg_version.restype = C.c_char_p
    sig = {
        "pg_device_count": [P(i32)],
        "pg_model_num_outputs": [vp, P(u32)],
        "pg_model_f16_stats": [vp, P(C.c_uint64)],
        "pg_init": [i32, vp, P(vp)],
        "pg_shutdown": [vp],
        "pg_synchronize": [vp],
        "pg_device_malloc": [vp, sz, P(vp)],
        "pg_device_free": [vp, vp],
        "pg_memcpy_h2d": [vp, vp, vp, sz],
        "pg_memcpy_d2h": [vp, vp, vp, sz],
        "pg_table_create": [vp, u64, u32, u64, P(vp)],
        "pg_table_destroy": [vp, vp],
        "pg_table_fill_synthetic": [vp, vp, u64, i32],
        "pg_table_upload": [vp, vp, u64, u64, vp],
        "pg_table_download": [vp, vp, u64, u64, vp],
        "pg_table_swap": [vp, vp, vp],
        "pg_table_info": [vp, P(u64), P(u32), P(u64)],
        "pg_table_gather": [vp, vp, vp, u32, vp],
        "pg_recall_topk": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_recall_topk_dev": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_recall_topk_l2": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_recall_topk_l2_dev": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_recall_topk_where": [vp, vp, vp, i32, i32, C.c_longlong, i32, vp, u32, u32, vp, vp, vp],
        "pg_table_view_create": [vp, vp, vp, i32, i32, C.c_longlong, vp],
        "pg_index_build": [vp, vp, P(PgIndexParams), P(vp)],
        "pg_index_destroy": [vp, vp],
        "pg_index_recall_topk": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_index_recall_topk_dev": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_index_recall_topk_l2": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_index_recall_topk_l2_dev": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_index_stats": [vp, P(PgIndexStats)],
        "pg_index_attach": [vp, vp],
        "pg_index_detach": [vp, vp],
        "pg_index_serving_stats": [vp, P(PgIndexServingStats)],
        "pg_index_recall_topk_where": [vp, vp, vp, i32, i32, C.c_longlong, i32, vp, u32, u32, vp, vp, vp],
        "pg_index_where_read": [vp, vp, vp, i32, i32, C.c_longlong, vp, vp, vp],
        "pg_index_where_stats": [vp, P(PgIndexWhereStats)],
        "pg_where_compile": [C.c_char_p, P(vp)],
        "pg_where_free": [vp],
        "pg_where_num_columns": [vp],
        "pg_where_eval_host": [vp, P(vp), P(i32), C.c_uint64, vp],
        "pg_recall_topk_where_ex": [vp, vp, vp, vp, i32, vp, u32, u32, vp, vp, vp],
        "pg_index_recall_topk_where_ex": [vp, vp, vp, vp, i32, vp, u32, u32, vp, vp, vp],
        "pg_table_view_create_ex": [vp, vp, vp, vp, P(vp)],
        "pg_where_bits": [vp, vp, vp, C.c_uint64, vp, P(C.c_uint64)],
        "pg_where_stats": [vp, P(PgWhereStats)],
        "pg_exclude_compact_dev": [vp, vp, vp, u32, u32, vp, vp, u32, C.c_float, vp, vp, vp],
        "pg_cold_create": [vp, C.c_char_p, P(vp)],
        "pg_cold_free": [vp],
        "pg_cold_recall_host": [vp, vp, u64, u64, vp, i32, vp, u32, u32, vp, vp, vp],
        "pg_cold_recall_dev": [vp, vp, vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_cold_recall": [vp, vp, vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_cold_stats": [vp, P(PgColdStats)],
        "pg_recall_topk_exclude": [vp, vp, vp, u32, u32, vp, vp, P(PgRecallExcludeOpts), vp, vp, vp],
        "pg_recall_topk_exclude_dev": [vp, vp, vp, u32, u32, vp, vp, P(PgRecallExcludeOpts), vp, vp, vp],
        "pg_i2i_recall_exclude": [vp, vp, vp, u32, vp, u32, i32, vp, vp, vp, vp, vp],
        "pg_coalescer_recall_exclude": [vp, vp, vp, u32, vp, vp, P(u32)],
        "pg_simtable_create": [vp, vp, P(vp)],
        "pg_simtable_upload": [vp, vp, u64, u64, vp, vp, vp],
        "pg_simtable_info": [vp, P(u64), P(u64), P(u64), P(u64)],
        "pg_simtable_destroy": [vp, vp],
        "pg_cf_recall": [vp, vp, vp, vp, vp, u32, u32, P(PgCfOpts), vp, vp, vp],
        "pg_cf_recall_dev": [vp, vp, vp, vp, vp, u32, u32, P(PgCfOpts), vp, vp, vp],
        "pg_rtu2i_compile": [P(PgRtU2IConf), P(vp)],
        "pg_rtu2i_free": [vp],
        "pg_rtu2i_trigger_count": [vp],
        "pg_rtu2i_triggers_host": [vp, u64, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp],
        "pg_rtu2i_triggers": [vp, vp, u64, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp],
        "pg_rtu2i_triggers_dev": [vp, vp, u64, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp],
        "pg_rtu2i_expand": [vp, vp, vp, vp, vp, u32, u32, P(PgCfOpts), vp, vp, vp],
        "pg_rtu2i_expand_dev": [vp, vp, vp, vp, vp, u32, u32, P(PgCfOpts), vp, vp, vp],
        "pg_rtu2i_recall": [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, P(PgCfOpts), vp, vp, vp],
        "pg_rtu2i_recall_dev": [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, P(PgCfOpts), vp, vp, vp],
        "pg_xtable_create": [vp, vp, u32, P(vp)],
        "pg_xtable_upload_item2x": [vp, vp, u64, u64, vp, vp],
        "pg_xtable_upload_x2item": [vp, vp, u32, u32, vp, vp, vp],
        "pg_xtable_info": [vp, P(u64), P(u32), P(u64), P(u64), P(u64)],
        "pg_xtable_destroy": [vp, vp],
        "pg_x2i_recall": [vp, vp, vp, vp, vp, u32, u32, P(PgX2iOpts), vp, vp, vp],
        "pg_x2i_recall_dev": [vp, vp, vp, vp, vp, u32, u32, P(PgX2iOpts), vp, vp, vp],
        "pg_x2i_recall_host": [u64, u64, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, P(PgX2iOpts), vp, vp, vp],
        "pg_rtu2i_x_recall": [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, P(PgX2iOpts), vp, vp, vp],
        "pg_rtu2i_x_recall_dev": [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, P(PgX2iOpts), vp, vp, vp],
        "pg_bloom_estimate": [u64, C.c_double, P(u64), P(u32)],
        "pg_bloom_murmur3_host": [vp, u64, u32, P(u32)],
        "pg_bloom_keys_create": [vp, u64, vp, vp, P(vp)],
        "pg_bloom_keys_create_decimal": [vp, u64, vp, P(vp)],
        "pg_bloom_keys_free": [vp, vp],
        "pg_bloom_create": [vp, u64, u32, vp, u32, P(vp)],
        "pg_bloom_free": [vp, vp],
        "pg_bloom_info": [vp, P(u64), P(u32), P(u32), P(u64)],
        "pg_bloom_slot_write": [vp, vp, u32, vp, u64],
        "pg_bloom_slot_read": [vp, vp, u32, vp, u64],
        "pg_bloom_slot_clear": [vp, vp, u32],
        "pg_bloom_exists_dev": [vp, vp, vp, u32, u32, vp, vp, vp, vp],
        "pg_bloom_filter_dev": [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp],
        "pg_bloom_add_dev": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_bloom_exists": [vp, vp, vp, u32, vp, u32, vp],
        "pg_bloom_filter": [vp, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp],
        "pg_bloom_add": [vp, vp, vp, u32, vp, u32],
        "pg_bloom_exists_host": [u64, u32, vp, u32, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp],
        "pg_bloom_add_host": [u64, u32, vp, u32, vp, u64, vp, vp, u32, u32, vp, vp, vp],
        "pg_bloom_filter_host": [u64, u32, vp, u32, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp,
                                 vp, vp, vp],
        "pg_bloom_slot_write_host": [u64, u32, vp, u32, vp, u64],
        "pg_hottable_create": [vp, vp, u32, P(vp)],
        "pg_hottable_upload": [vp, vp, u32, u32, vp, vp, vp, vp],
        "pg_hottable_info": [vp, P(u64), P(u32), P(u64), P(u32), P(u64)],
        "pg_hottable_destroy": [vp, vp],
        "pg_hot_recall_dev": [vp, vp, C.c_int, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp],
        "pg_hot_recall": [vp, vp, C.c_int, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp],
        "pg_hot_recall_host": [u64, u64, u32, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp],
        "pg_fanin_merge_dev": [vp, P(PgFaninSource), u32, u32, vp, vp, vp, vp, vp, vp],
        "pg_recommend_candidates_dnn3_dev": [vp, vp, vp, vp, C.c_char_p, vp, u32, u32, vp, vp, vp, vp, vp, vp],
        "pg_trim_out_cap": [P(PgTrimRule), u32, u32, P(C.c_uint32)],
        "pg_candidates_trim_dev": [vp, P(PgTrimRule), u32, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_trim2_out_cap": [P(PgTrimRule), u32, u32, P(C.c_uint32)],
        "pg_candidates_trim2_dev": [vp, P(PgTrimRule), u32, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_candidates_trim2_host": [P(PgTrimRule), u32, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_blend_out_cap": [P(PgBlendConf), u32, P(C.c_uint32)],
        "pg_candidates_blend_dev": [vp, P(PgBlendConf), u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_candidates_blend_host": [P(PgBlendConf), u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_recommend_cascade_dnn3_dev": [vp, vp, vp, vp, C.c_char_p, vp, vp, C.c_char_p, vp, u32, u32, vp, vp, vp, vp, u32,
                                          vp, vp, vp, vp, vp, vp, vp],
        "pg_diversity_rules_host": [P(PgDivConfig), u32, u32, vp, vp, vp, vp, vp],
        "pg_diversity_rules_dev": [vp, P(PgDivConfig), u32, u32, vp, vp, vp, vp, vp],
        "pg_diversity_rules_features_dev": [vp, P(PgDivConfig), vp, P(C.c_char_p), u32, u32, vp, vp, vp, vp, vp],
        "pg_diversity_rules": [vp, P(PgDivConfig), u32, vp, vp, vp],
        "pg_expr_compile_govaluate": [C.c_char_p, P(vp)],
        "pg_expr_eval_host": [vp, vp, u32, vp],
        "pg_cond_compile": [P(PgCondRule), u32, P(PgCondCol), u32, u32, P(vp)],
        "pg_cond_free": [vp],
        "pg_cond_num_rules": [vp],
        "pg_cond_num_user_slots": [vp],
        "pg_cond_user_slot_is_float": [vp, i32],
        "pg_cond_match_host": [vp, u32, u32, vp, P(vp), vp, u32, vp],
        "pg_boost_scores_host": [vp, u32, u32, vp, P(vp), vp, u32, vp, vp, vp],
        "pg_item_state_filter_dev": [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "pg_boost_scores_dev": [vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_item_state_filter": [vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp],
        "pg_boost_scores": [vp, vp, u32, u32, vp, P(vp), vp, u32, vp, vp, vp],
        "pg_distinct_ids_host": [vp, vp, u32, vp, P(vp), vp, u32, vp],
        "pg_distinct_ids_dev": [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp],
        "pg_distinct_ids": [vp, vp, vp, u32, vp, P(vp), vp, u32, vp],
        "pg_candidates_dimcap_host": [P(PgDimcapConf), u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_candidates_dimcap_dev": [vp, vp, P(PgDimcapConf), u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_candidates_dimcap": [vp, vp, P(PgDimcapConf), u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_classcut_compile": [P(PgClasscutRule), u32, P(PgCondCol), u32, P(C.c_char_p), u32, P(vp)],
        "pg_classcut_free": [vp],
        "pg_classcut_num_classes": [vp],
        "pg_classcut_reads_recall_name": [vp],
        "pg_classcut_out_cap": [vp, u32, P(C.c_uint32)],
        "pg_classcut_masks_host": [vp, u32, vp, P(vp), vp, vp, vp],
        "pg_candidates_classcut_host": [vp, u32, u32, vp, P(vp), vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_classcut_masks_dev": [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp],
        "pg_candidates_classcut_dev": [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_candidates_classcut": [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp],
        "pg_mix_compile": [P(PgMixStrategy), u32, P(PgCondCol), u32, u32, u32, P(vp)],
        "pg_mix_free": [vp],
        "pg_mix_num_strategies": [vp],
        "pg_mix_num_user_slots": [vp],
        "pg_mix_user_slot_is_float": [vp, i32],
        "pg_mix_sort_host": [vp, u32, u32, u32, vp, P(vp), vp, vp, vp, vp, vp, vp, vp, vp],
        "pg_mix_sort_dev": [vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "pg_mix_sort": [vp, vp, vp, u32, u32, vp, vp, vp, u64, vp, u32, vp, P(u32)],
        "pg_traffic_compile": [P(PgTrafficTarget), u32, P(vp)],
        "pg_traffic_free": [vp],
        "pg_traffic_num_targets": [vp],
        "pg_traffic_table": [i32, u32, u32, vp],
        "pg_traffic_sort_host": [vp, u32, u32, C.c_double, C.c_double, C.c_double, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "pg_traffic_sort_dev": [vp, vp, u32, u32, C.c_double, C.c_double, C.c_double, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "pg_traffic_sort": [vp, vp, u32, u32, C.c_double, C.c_double, C.c_double, u32, vp, vp, vp, vp, vp, P(u32), vp, vp],
        "pg_ssd_sort_dev": [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, C.c_double, u32, u32, i32, i32, i32, i32, u32, C.c_double, u32, u32,
                            vp, vp, vp, vp],
        "pg_index_refresh": [vp, vp, P(PgIndexRefreshParams)],
        "pg_index_refresh_stats": [vp, P(PgIndexRefreshStats)],
        "pg_index_screen_probe": [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp],
        "pg_index_read": [vp, vp, vp, vp, vp, vp, vp],
        "pg_index_bounds": [vp, vp, vp, u32, i32, vp],
        "pg_topk_merge_dev": [vp, vp, vp, u32, u32, u32, u32, vp, vp],
        "pg_model_load": [vp, i32, i32, vp, sz, P(vp)],
        "pg_model_destroy": [vp, vp],
        "pg_rank_dnn3": [vp, vp, vp, vp, vp, vp, u32, vp],
        "pg_rank_dnn3_dev": [vp, vp, vp, vp, vp, vp, u32, u32, vp],
        "pg_rank_fm2t": [vp, vp, vp, vp, vp, vp, u32, vp],
        "pg_rank_fm2t_dev": [vp, vp, vp, vp, vp, vp, u32, u32, vp],
        "pg_expr_compile": [C.c_char_p, P(vp)],
        "pg_expr_free": [vp],
        "pg_expr_num_vars": [vp],
        "pg_expr_set_score_rewrites": [vp, u32, vp, vp],
        "pg_expr_compile_typed": [C.c_char_p, C.c_char_p, P(vp)],
        "pg_expr_is_antlr": [vp],
        "pg_fuse_scores_dev": [vp, vp, vp, u32, vp, sz, vp, u32, vp],
        "pg_expr_eval": [vp, vp, vp, u32, vp],
        "pg_expr_eval_dev": [vp, vp, vp, u32, vp],
        "pg_sort_scores": [vp, vp, vp, u32, i32, vp],
        "pg_sort_scores_dev": [vp, vp, vp, u32, u32, u32, i32, vp],
        "pg_dpp": [vp, vp, vp, vp, u32, C.c_double, u32, u32, i32, vp, vp],
        "pg_dpp_ex": [vp, vp, vp, vp, u32, P(PgDppOptions), vp, vp, vp, vp],
        "pg_ssd": [vp, vp, vp, vp, u32, C.c_double, u32, u32, i32, i32, i32, i32, vp, vp, vp],
        "pg_ssd_emb": [vp, vp, u32, vp, u32, C.c_double, u32, u32, i32, i32, i32, i32, vp, vp, vp],
        "pg_features_create": [vp, u64, P(vp)],
        "pg_features_destroy": [vp, vp],
        "pg_features_set_column": [vp, vp, C.c_char_p, i32, vp, C.c_double],
        "pg_features_column_index": [vp, C.c_char_p],
        "pg_features_num_columns": [vp],
        "pg_features_gather_i32_dev": [vp, vp, vp, u32, vp, u32, vp],
        "pg_features_gather_f32_dev": [vp, vp, vp, u32, vp, vp, vp, u32, vp],
        "pg_rank_fm2t_rows_dev": [vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp],
        "pg_rank_fm2t_rows": [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp],
        "pg_recommend_dnn3_dev": [vp, vp, vp, vp, C.c_char_p, vp, u32, u32, vp, vp, vp, vp, vp, vp],
        "pg_set_option": [vp, C.c_char_p, C.c_char_p],
        "pg_table_fill_gaussian": [vp, vp, u64, C.c_float],
        "pg_table_fill_mixture": [vp, vp, u64, C.c_uint32, C.c_float],
        "pg_i2i_recall": [vp, vp, vp, u32, vp, u32, vp, vp, vp],
        "pg_online_vector_recall": [vp, vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_fm2t_user_embedding": [vp, vp, vp, u32, vp],
        "pg_fm2t_user_embedding_dev": [vp, vp, vp, u32, vp],
        "pg_recommend_dnn3_begin": [vp, vp, vp, vp, C.c_char_p, vp, u32, u32, vp, vp, vp, vp, vp, vp, P(vp)],
        "pg_recommend_end": [vp, vp, P(C.c_double)],
        "pg_coalescer_create": [vp, vp, vp, vp, C.c_char_p, P(PgCoalescerConfig), P(vp)],
        "pg_coalescer_destroy": [vp],
        "pg_coalescer_recall": [vp, vp, vp, vp, P(u32)],
        "pg_coalescer_rank_dnn3": [vp, vp, vp, u32, vp],
        "pg_coalescer_recommend": [vp, vp, u32, vp, vp, vp, vp, P(u32)],
        "pg_coalescer_stats": [vp, P(PgCoalescerStats)],
        "pg_coalescer_create_scene": [vp, vp, P(PgSceneConfig), P(vp)],
        "pg_coalescer_i2i_recall": [vp, u32, vp, vp, P(u32)],
        "pg_coalescer_recall_l2": [vp, vp, vp, vp, P(u32)],
        "pg_coalescer_online_recall": [vp, vp, vp, vp, P(u32)],
        "pg_coalescer_rank": [vp, u32, vp, vp, vp, u32, vp],
        "pg_coalescer_rank_fm2t": [vp, vp, vp, vp, u32, vp],
        "pg_coalescer_recommend_ex": [vp, vp, vp, u32, vp, vp, vp, vp, P(u32)],
        "pg_coalescer_dpp": [vp, vp, vp, u32, P(PgDppOptions), vp, vp, P(u32), vp],
        "pg_coalescer_ssd": [vp, vp, vp, u32, C.c_double, u32, u32, i32, i32, i32, i32, vp, P(u32), vp],
        "pg_recommend_end_timed": [vp, vp, u32, P(C.c_double)],
        "pg_debug_stall": [vp, u32],
        "pg_fm2t_item_rows_build": [vp, vp, vp, vp, P(vp)],
        "pg_fm2t_item_rows_update": [vp, vp, u64, u64],
        "pg_fm2t_item_rows_destroy": [vp, vp],
        "pg_rank_fm2t_irows_dev": [vp, vp, vp, vp, vp, vp, vp, u32, u32, vp],
        "pg_rank_fm2t_irows": [vp, vp, vp, vp, vp, vp, vp, u32, vp],
        "pg_topk_merge_lists_dev": [vp, vp, vp, u32, u32, u32, i32, u32, vp, vp],
        "pg_owned_compact_dev": [vp, vp, vp, u32, u32, vp, vp, vp],
        "pg_scatter_f32_dev": [vp, vp, vp, vp, u32, vp],
        "pg_dpp_candidates_dev": [vp, vp, vp, vp, u32, u32, u32, vp, vp],
        "pg_gather_owned_rows_dev": [vp, vp, vp, u32, vp],
        "pg_dpp_batch_dev": [vp, vp, vp, u32, u32, u32, C.c_double, u32, u32, i32, vp, vp],
        "pg_dpp_kernel_matrix_dev": [vp, vp, vp, u32, u32, u32, C.c_double, i32, vp],
        "pg_features_eval_dev": [vp, vp, vp, vp, u32, vp],
        "pg_group_create": [P(C.c_int), u32, P(vp)],
        "pg_group_destroy": [vp],
        "pg_group_table_create": [vp, u64, u32],
        "pg_group_table_fill_synthetic": [vp, u64, i32],
        "pg_group_table_upload": [vp, u64, u64, vp],
        "pg_group_model_load": [vp, i32, i32, vp, sz],
        "pg_group_recommend": [vp, vp, C.c_char_p, P(PgGroupPlan), vp, u32, u32, vp, vp, vp, vp, vp],
        "pg_group_recommend_begin": [vp, vp, C.c_char_p, P(PgGroupPlan), vp, u32, u32, P(vp)],
        "pg_group_recommend_end": [vp, vp, vp, vp, vp, vp, vp],
        "pg_group_info": [vp, P(u64), P(u32)],
        "pg_group_exchange_stats": [vp, P(u64)],
        "pg_coalescer_create_group": [vp, vp, C.c_char_p, P(PgGroupPlan), P(PgCoalescerConfig), P(vp)],
        "pg_router_create": [P(vp), u32, P(vp)],
        "pg_router_destroy": [vp],
        "pg_router_recommend": [vp, vp, u32, vp, vp, vp, vp, P(u32)],
        "pg_router_recall": [vp, vp, vp, vp, P(u32)],
        "pg_router_stats": [vp, P(u64)],
        "pg_rows_to_local_dev": [vp, vp, vp, u32, vp, vp],
        "pg_widen_f32_dev": [vp, vp, u32, vp],
        "pg_stats": [vp, P(PgStats)],
        "pg_last_scan_kernel_ms": [vp, P(C.c_double), P(u64)],
        "pg_hbm_read_probe": [vp, vp, i32, P(C.c_double)],
        "pg_table_screen_info": [vp, vp, P(C.c_int), P(C.c_float), P(C.c_float)],
        "pg_table_derived_info": [vp, vp, u32, P(PgTableDerived)],
        "pg_table_derived_read": [vp, vp, i32, u64, u64, vp],
    }
    missing = [n for n in EXPORTS if not hasattr(L, n)]
    if missing:
        raise ImportError("pairec_amd: %s lacks symbols %s declared in include/pairec_gpu.h "
                          "(stale build?)" % (LIB_PATH, missing))
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = i32
    L.pg_group_size.argtypes = [vp]
    L.pg_group_size.restype = u32
    L.pg_group_ctx.argtypes = [vp, u32]
    L.pg_group_ctx.restype = vp
    L.pg_group_table.argtypes = [vp, u32]
    L.pg_group_table.restype = vp
    L.pg_expr_var_name.argtypes = [vp, i32]
    L.pg_expr_var_name.restype = C.c_char_p
    L.pg_where_column_name.argtypes = [vp, i32]
    L.pg_where_column_name.restype = C.c_char_p
    L.pg_cond_user_slot_name.argtypes = [vp, i32]
    L.pg_cond_user_slot_name.restype = C.c_char_p
    L.pg_mix_user_slot_name.argtypes = [vp, i32]
    L.pg_mix_user_slot_name.restype = C.c_char_p
    _lib = L
    return L


class PgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("pairec_gpu error %d: %s" % (code, msg))
        self.code = code


def check(rc: int):
    if rc != 0:
        raise PgError(rc, load().pg_last_error().decode("utf-8", "replace"))
