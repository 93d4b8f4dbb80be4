// recall_shared.hpp — what more than one of recall.hip, recall_plan.hip, recall_select.hip, recall_table.hip, recall_filter.hip
// and recall_entry.hip needs and no file outside them does (what other files call is declared in common.hpp).
#pragma once
#include "common.hpp"
#include "recall_plan_math.hpp"      // kPieceRows, kCandSlack, kRecBytes, kRecPoolSlice, next_pow2

namespace pg {

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
// The bf16 screen's margin is kScreenEps ||q|| x the largest row norm of the block, read from an fp32 sum of squares.  Below this
// norm that sum is not to be trusted — d squares that underflow lose up to d 2^-126 = 1.5e-36 of it, 1.5e-4 of 1e-32, which the
// 1.0002 on the norm still covers; a sum of 1e-40 can have lost everything — and the screen takes the floor instead.
constexpr float kScreenNormFloor = 1e-16f;
static_assert(kRecQueries == (uint32_t)kMaxQueries, "recall_plan_math.hpp sizes the hit-record areas for kMaxQueries queries");

// ---- the table pass (recall.hip) as the plans (recall_plan.hip) see it: the arguments of a launch and the launchers.  A launcher
// owns the choice of the kernel's instantiation and its grid.
constexpr int kScreenMaxNQB = 8;                // 8 x 32 = 256 queries per pass at most
constexpr uint32_t kRecOvfWord = 1 + kMaxQueries + 1;       // rs.overflow[kRecOvfWord]: the overflow was one of the hit-record areas (they can grow: TableLearned::rec_scale)

struct ScanArgs {
    const float* tab;        // [rows][DIM]
    const float* qpad;       // [32][DIM] queries, zero-padded
    const float* thr;        // [32] running thresholds
    uint32_t* cnt;           // [32] candidate counts
    uint64_t* cand;          // [32][cap] candidate keys
    uint32_t* overflow;      // set to 1 if any list overflowed
    uint32_t cap;
    uint32_t nq;
    uint32_t nq_launch;      // queries of the call (selects the 32- or 64-query kernel)
    uint32_t rb_begin;       // first 32-row block of this launch
    uint32_t rb_end;         // one past the last block
    uint32_t row_end;        // rows >= row_end are ignored (table end)
    uint32_t stride;         // 1 = every block; S > 1 = pilot sample: logical block L reads table
                             // block sample_block(L, ...)
    uint32_t perm_mul, perm_mod;   // pilot sample order: slot = L * perm_mul mod perm_mod
    uint32_t group_q;        // > 0: blockIdx.y selects a group of group_q queries (of nq in all) — one launch serves
                             // every group of a screened recall's exact seed scan instead of one launch per group
    // squared-Euclidean recall (scan_kernel<…, L2 = true>): a row·query pair is ranked by -d = fmaf(2, ip, -(|x|^2 + |q|^2))
    const float* nx;         // [rows + 64] |x|^2 of every row (k-ascending fmaf chain; TableDerived::d_nx)
    const float* nqv;        // [nq] |q|^2 of every query
    RowFilter filter;        // rows that fail it are no candidates (col = nullptr: none)
};

struct ScreenArgs {
    const void* tab16;        // shadow of the table: bf16 (TableDerived::d16) or int8 (TableDerived::d8)
    const uint4* qb16;        // [NQB][KS][64] B fragments: 8 bf16 (KS = DIM/16) or 16 int8 (KS = DIM/32) per lane
    const float* thr_screen;  // [256] bf16: thr - eps, rounded down; int8: the same in integer dot units (int32 bits)
    uint32_t* susp_cnt;       // [256] suspects per query of this launch
    uint32_t* susp;           // [256][cap] suspect rows (passed the screen; re-scored by rescore_kernel)
    uint32_t* overflow;
    uint32_t cap, nq, rb_begin, rb_end, row_end, stride, perm_mul, perm_mod;
    // bf16 only: the bound is relative to the row's norm — eps = eps_unit[q] x (largest row norm of the 32-row block)
    const float* blk_norm2;   // [blocks] largest row norm^2 per physical 32-row block (TableDerived::dnorm2)
    const float* eps_unit;    // [256] 0.008 ||q|| (inflated); thr_screen then carries thr itself (or -inf)
    // query halves (int8, > 128 queries): hit records instead of staged (row, query) pairs — see kRecBytes
    char* rec = nullptr;      // [waves][rec_cap] records of kRecBytes: one region per wave of the launch
    uint32_t* rec_cnt = nullptr;   // [waves] records in each region (zeroed per launch); [waves]: records in the spill pool
    uint32_t rec_cap = 0;
    char* rec_pool = nullptr; // [rec_pool_cap] records: where a wave whose region is full puts its staged records
    uint32_t rec_pool_cap = 0, rec_waves = 0;
    uint32_t early_share = 512;    // 8-wave variants: share (x 1024) of a SIMD's blocks that goes to its older wave; 512 = even
    // squared-Euclidean recall on the int8 screen (L2 = true, <= 128 queries): a pair is a suspect iff
    // I >= floor(A_q + B_q * min|x|^2 of the block) - 2, with thr_screen = A_q (float) and l2_b = B_q (screen_thr8_l2_kernel)
    const float* blk_nxmin = nullptr;   // [blocks] smallest |x|^2 of every physical 32-row block (TableDerived::d_nxmin)
    const float* l2_b = nullptr;        // [256]
    const float* nx_rows = nullptr;     // L2 = 2 (per-row test: g = 2 s_x s_q I - |x|^2 >= C'_q, thr_screen = C'_q, l2_b = 2 s_x s_q): |x|^2 of every row
};

int dispatch_scan(pg_ctx* ctx, uint32_t dim, const ScanArgs& a);
// the screened launch; with hit records in use (a.rec) screen_decode_kernel turns them into the suspect lists right behind it
int screen_launch(pg_ctx* ctx, uint32_t dim, bool i8, const ScreenArgs& a);
// per plan: the queries' B fragments, eps and scales in the shadow's format (wide: the > 128-query int8 pass's query halves)
int screen_prep_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, uint32_t nq, bool wide);
// rs.thr → the screen's own units in rs.thr_screen: the squared-Euclidean, int8 or bf16 form (l2: + B_q in rs.thr_ref, |q|^2 from rs.pred_ms)
int screen_thr_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, bool l2, bool l2_per_row);

// recall_table.hip.  What it builds lives in pg_table::derived, what the plans learn from verified batches in pg_table::learned;
// g_table_state_mu guards both, and `learned` is read through table_learned()'s snapshots only (table_state.hpp, common.hpp).
int ensure_pred_model(pg_ctx* ctx, const pg_table* t);       // builds the threshold model once per generation of the rows (dim 128)
// recall_filter.hip (caller holds ctx->mu; one launch each, nothing synchronises): *d_n += the rows of [0, rows) that `filter`
// admits; d_rows[i] = offset + ids[d_rows[i]] for the n entries below `rows` (local rows of a compact table → the source's)
int filter_count_launch(pg_ctx* ctx, const RowFilter& filter, uint64_t rows, unsigned long long* d_n);
int compact_map_rows_launch(pg_ctx* ctx, uint64_t* d_rows, uint64_t n, const uint32_t* ids, uint64_t offset, uint64_t rows);

}  // namespace pg
