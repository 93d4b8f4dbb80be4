// recall_shared.hpp — what more than one of recall.hip, recall_select.hip, recall_table.hip, recall_filter.hip and
// recall_entry.hip needs and no file outside them does (what other files call is declared in common.hpp).
#pragma once
#include "common.hpp"

namespace pg {

// rows of a block of the table pass (recall.hip), the unit of a table's per-block data (recall_table.hip)
constexpr int kPieceRows = 32;

// The 64-bit candidate key: score descending (IEEE totalOrder, NaN last), then row ascending.

__device__ __forceinline__ uint32_t f32_ordered_bits(float f) {
    const uint32_t b = __float_as_uint(f);
    if (f != f) return 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint64_t topk_key(float score, uint32_t row) {
    return ((uint64_t)f32_ordered_bits(score) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ float key_score(uint64_t key) {
    const uint32_t ob = (uint32_t)(key >> 32);
    if (ob == 0u) return __uint_as_float(0x7FC00000u);
    const uint32_t b = (ob & 0x80000000u) ? (ob & 0x7FFFFFFFu) : ~ob;
    return __uint_as_float(b);
}
__device__ __forceinline__ uint32_t key_row(uint64_t key) {
    return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu);
}

constexpr float kScreenEps = 0.008f;
constexpr uint32_t kCandSlack = 1u << 19;      // candidate capacity beyond K per query

static uint32_t next_pow2(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// recall_table.hip.  What it builds lives in pg_table::derived, what the plans learn from verified batches in pg_table::learned;
// g_table_state_mu guards both, and `learned` is read through table_learned()'s snapshots only (table_state.hpp, common.hpp).
int ensure_pred_model(pg_ctx* ctx, const pg_table* t);       // builds the threshold model once per generation of the rows (dim 128)
// recall_filter.hip (caller holds ctx->mu; one launch each, nothing synchronises): *d_n += the rows of [0, rows) that `filter`
// admits; d_rows[i] = offset + ids[d_rows[i]] for the n entries below `rows` (local rows of a compact table → the source's)
int filter_count_launch(pg_ctx* ctx, const RowFilter& filter, uint64_t rows, unsigned long long* d_n);
int compact_map_rows_launch(pg_ctx* ctx, uint64_t* d_rows, uint64_t n, const uint32_t* ids, uint64_t offset, uint64_t rows);

}  // namespace pg
