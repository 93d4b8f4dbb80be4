"""pairec_amd — MI355X-native engine for pairec's rank + recall hot path.

The product is libpairec_gpu.so (C ABI, include/pairec_gpu.h) built from pairec_amd/csrc.
This package is the Python host mirror used by tests and bench.py; see INTEGRATION.md for the
cgo shim that plugs the same library under pairec's algorithm/recall/sort registries.
"""
from . import _lib  # noqa: F401
from .engine import (Context, Table, SimTable, XTable, x2i_recall_host, HotTable, hot_recall_host, RtU2I, Index, index_screen_probe, RankModel, Expr, Where, ColdStart, Bloom, BloomKeys, bloom_estimate, bloom_murmur3_host, bloom_pack_keys, bloom_exists_host, bloom_add_host, bloom_filter_host, bloom_slot_write_host, Features, ItemRows, Coalescer, GroupCoalescer, Router, ShardGroup, recommend_dnn3, recommend_candidates_dnn3, recommend_cascade_dnn3, trim_out_cap, trim2_out_cap, candidates_trim2_host, blend_out_cap, candidates_blend_host, diversity_rules_host, Cond, cond_compile, cond_match_host, distinct_ids_host, candidates_dimcap_host, Classcut, classcut_compile, classcut_out_cap, classcut_masks_host, candidates_classcut_host, Mix, mix_compile, mix_sort_host, Traffic, traffic_compile, traffic_sort_host, traffic_table, expr_compile_govaluate, dpp, dpp_ex, ssd, ssd_emb, pack_dnn3, pack_dnn3_multi, pack_fm2t,  # noqa: F401
                     F_I32, F_I64, F_F32, F_F64, TRIM_FIX, TRIM_ACCUMULATE, TRIM_ANY, BLEND_SNAKE_REFILL, BLEND_SNAKE_SKIP, BLEND_FAIR,
                     DIV_MAX_N, DIV_MAX_RULES, DIV_MAX_DIMS, DIV_MAX_COLS, DIV_MAX_EXCL, DIV_MAX_TERMS, DIV_MAX_POSITIONS, DIV_CHUNK,
                     COND_MAX_RULES, COND_MAX_TERMS, COND_MAX_COLS, COND_MAX_SLOTS, COND_MAX_LIST,
                     HOT_GROUP, HOT_GLOBAL, HOT_TOPIC, HOT_MAX_ENTRIES, HOT_UNSCORED, HOT_PAD_SOURCE,
                     BLOOM_MAX_KEY, BLOOM_MAX_K, BLOOM_NO_SLOT, DIMCAP_NULL_KEEP, DIMCAP_NULL_VALUE, DIMCAP_CHUNK, DIMCAP_MIN_SLOTS, DIMCAP_LDS_MAX_CAP,
                     MIX_FIX, MIX_RANDOM, MIX_MAX_STRATEGIES, MIX_MAX_POSITIONS, MIX_MAX_SIZE,
                     TRAFFIC_PERCENT, TRAFFIC_QUANTITY, TRAFFIC_MAX_TARGETS,
                     WHERE_GT, WHERE_GE, WHERE_LT, WHERE_LE, WHERE_EQ, WHERE_NE,
                     PREC_F32, PREC_BF16, PREC_BF16X3, PREC_F16X2, PREC_F16, MODEL_DNN3, MODEL_FM_TWOTOWER, MODEL_DNN3_MULTI, MAX_QUERIES)
