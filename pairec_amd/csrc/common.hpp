// common.hpp — shared host-side plumbing of libpairec_gpu.so (context, error convention).
// gfx950 (MI355X) only: wave = 64 lanes, 256 CUs, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <atomic>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/pairec_gpu.h"
#include "scratch_layout.hpp"
#include "table_state.hpp"
#include "rank_model.hpp"     // pg_model

namespace pg {

struct PipeRun;          // pipeline.hpp
void set_error(const char* fmt, ...);

#define PG_HIP(expr)                                                                           \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            ::pg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__,  \
                            __LINE__);                                                         \
            return PG_ERR_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

#define PG_REQUIRE(cond, ...)                    \
    do {                                         \
        if (!(cond)) {                           \
            ::pg::set_error(__VA_ARGS__);        \
            return PG_ERR_INVALID;               \
        }                                        \
    } while (0)

constexpr int kWave = 64;
constexpr int kMaxQueriesExact = 64;   // exact fp32-MFMA scan: one or two 32-query column blocks
constexpr int kMaxQueries = 256;       // screened scan (int8 or bf16 filter + exact rescoring): up to eight blocks

// Scratch arena: grows on demand, never shrinks; owned by the context, used by one call at a time
// (calls on a context are serialised by ctx->mu).
struct Scratch {
    void* p = nullptr;
    size_t cap = 0;
};
// The arena's slots.  A slot's contents are valid until the next reserve of the same slot on this context; users that share a
// slot are stages that never hold it at the same time on the context's one stream.  The values are only array positions.
enum ScratchSlot : int {
    kSlotRows = 0,           // table.hip: the row ids of a gather from host rows; rank_mlp.hip: fm2t rows' gathered field ids (separate entry points, neither calls the other)
    kSlotHostStage = 1,      // table.hip: the gathered rows on their way to the host; features.hip: column descriptors and pointers of a gather (separate entry points)
    kSlotRecallSmall = 2,    // recall_plan.hip recall_scratch: padded queries, thresholds, counts, screen fragments, status words
    kSlotRecallCand = 3,     // recall_plan.hip recall_scratch: the candidate and suspect lists
    kSlotStatus = 4,         // 4096 bytes of status words (expr, misc, recall, recall_i4, recall_r2): each user writes, copies out and synchronises inside one step of its call
    kSlotStaging = 5,        // staging of every host-buffer entry point (rank, recall, sort, dpp, ssd, expr, cf, index, diversity): one per call under ctx->mu, synchronised before it returns
    kSlotRankTiles = 6,      // rank_mlp.hip: tile table + request partials
    kSlotWork = 7,           // work area of sort, split sort, dpp and ssd: each is one stage of a step, done with it before the next stage is enqueued on the stream
    kSlotPipe = 8,           // pipeline.hip post_scratch: the recommend pipeline's intermediates
    kSlotGroup = 9,          // group.hip pg_owned_compact_dev: the per-request counts of owned rows
    kSlotRerank = 10,        // pipeline.hip: the re-rank stage's DPP candidates
    kSlotHitRecords = 11,    // recall_plan.hip: the screened pass's record regions
    kSlotFilterCount = 12,   // recall_filter.hip filter_count_locked: per-block and per-group counts of the rows a filter admits
    kSlotFilterGather = 13,  // recall_filter.hip: the admitted rows' ids, compacted table and norms of a filtered recall
    kSlotRankHeads = 14,     // rank_mlp.hip: head partials of the weights-stationary multi-head kernel
    kSlotFuse = 15,          // pipeline.hip pg_fuse_scores_dev: the bound variables and error flags
    kSlotExprVars = 16,      // expr.hip pg_features_eval_dev: the bound variables
    kSlotIndexSearch = 17,   // index_search.hip: bounds, probe thresholds and list counts of an index recall; rank_mlp.hip: the fp16 split kernel's fallback tile tables (separate calls)
    kSlotRecallExclude = 18, // recall_entry.hip: the over-fetched answer, lists and counts of a recall with exclusion lists
    kSlotCf = 19,            // cf.hip: status and counts, staged offsets and lists, the global tier's tables, the items to order, the over-fetched answer
    kSlotFanin = 20,         // fanin.hip: the merge's keys, values and masks
    kSlotTrim = 21,          // trim.hip: segment offsets and the order of a coarse-rank cut
    kSlotCoarse = 22,        // pipeline.hip: the coarse stage's own outputs of a two-stage rank (fused scores, model scores, order)
    kSlotDiversity = 23,     // diversity.hip: keys, window counts and tuple tables
    kSlotDiversityPlanes = 24,  // diversity.hip: the dimension planes gathered from a feature store
    kSlotCond = 25,          // cond.hip: the one-request entries' staging (pg_item_state_filter, pg_boost_scores: inputs, outputs, the temporary store)
    kSlotBlend = 26,         // blend.hip: segment offsets, per-entry keys and orders, the compacted lists and the pick records
    kSlotClasscut = 27,      // classcut.hip: segment offsets, the score order and the class masks of a cut; the one-request entry's staging behind them
    kSlotTrim2 = 28,         // trim2.hip: segment offsets, per-rule keys and orders of a V2 quota cut
    kSlotMix = 29,           // mixsort.hip: the strategy masks and the taken lists of a mix sort; the one-request entry's staging behind them
    kSlotSsdStage = 30,      // ssd.hip pg_ssd_sort_dev: per-request counts and states, the position maps, the cut lists' rows and quality, the picks (kSlotWork stays the grid kernel's)
    kSlotDimcap = 31,        // dimcap.hip: the scratch tier's keys and counts of a value cap; the one-request entry's staging behind them
    kSlotRtU2I = 32,         // rtu2i.hip: the staged event offsets and clocks of a trigger stage; in pg_rtu2i_recall_dev the trigger lists between its two launches (cf.hip's expansion reads them while kSlotCf is its own)
    kSlotCold = 33,          // coldstart.hip: the select's threshold state and digit histogram, per-block counts and their scan, the survivors and the ordered list of an ordered pool
    kSlotTraffic = 34,       // traffic.hip: the position keys, the compacted lists, the keys' order, the list lengths and the segment offsets of a traffic control sort
    kSlotX2i = 35,           // x2i.hip: cf.hip's layout for a U2I2X2I recall — status and counts, staged offsets and lists, the global tier's tables, the items to order, the over-fetched answer (pg_rtu2i_x_recall's trigger lists are in kSlotRtU2I meanwhile)
    kSlotBloom = 36,         // bloom.hip: the probe's keep ballots of a Bloom filter call; the one-request entries' staging behind them
    kSlotHot = 37,           // hot.hip: the staged trigger offsets, sizes, ids and quotas of a list recall, behind them the sort records of the requests too long to order in LDS
    kSlotCount
};

// Developer / tuning knobs.  Read from the environment ONCE, in pg_init (a serving process must not change
// plans because of a stray variable later on, and getenv races with a host application's setenv); tests and
// A/B scripts change them per context with pg_set_option.
struct Knobs {
    uint32_t screen_min = 0;       // PG_SCREEN_MIN: batches up to this many queries use the exact scan
    bool recall_exact = false;     // PG_RECALL_EXACT: never screen
    double pilot_fraction = 0.0;   // PG_PILOT_FRACTION: sample fraction of the pilot plan (0 = default 1/64)
    bool no_pilot = false;         // PG_NO_PILOT: skip the pilot plan
    double pilot_sigmas = 6.0;     // PG_PILOT_SIGMAS: K' = m + sigmas sqrt(m) + 8 (margin of the pilot threshold)
    double chunk_growth = 0.0;     // PG_CHUNK_GROWTH: geometric growth of the grow plan (0 = default)
    uint32_t seed_rows = 8192;     // PG_SEED_ROWS: exact seed of the pilot sample
    double pilot_growth = 0.0;     // PG_PILOT_GROWTH: > 0 = geometric chunks over the sample instead of seed + one launch
    bool debug_scan = false;       // PG_DEBUG_SCAN: print per-launch times and suspect counts
    bool no_refine = false;        // PG_NO_REFINE: the pilot plan's full pass keeps the sample's threshold throughout
    uint32_t refine_min_rows = 1u << 24;   // PG_REFINE_MIN_ROWS: smallest table whose full pass is split for the refinement
    bool no_screen_i4 = false;     // PG_NO_SCREEN_I4: small batches stay on the int8 screen
    bool no_screen_i4m = false;    // PG_NO_SCREEN_I4M: batches of 5..64 queries stay on the int8 screen
    uint32_t i4m_min_queries = 1;  // PG_I4M_MIN_QUERIES: smallest batch it serves (below, and for squared-Euclidean recalls and tables without an int8 shadow: recall_i4.hip's vector-ALU screen, exact re-scoring of all its suspects; one query: 1.08 against 1.17 ms per 100 M rows)
    uint32_t i4m_max_queries = 64; // PG_I4M_MAX_QUERIES: largest batch the 4-bit matrix-pipe screen serves (<= kI4mMaxQueries)
    double i4m_max_lambda = 2.2;   // PG_I4M_MAX_LAMBDA: largest TableDerived::lam4 it is used for
    double i4m_max_pairs = 2.4e7;  // PG_I4M_MAX_PAIRS: ... and the most (row, query) pairs per pass its 4-bit stage may be expected to pass on
    uint32_t i4_min_rows = 1u << 22; // PG_I4_MIN_ROWS: smallest table the 4-bit screen is built for
    double i4_max_lambda = 1.7;    // PG_I4_MAX_LAMBDA: largest TableDerived::lam4 the 4-bit screen is used for
    bool rank_no_ws = false;       // PG_RANK_NO_WS: streaming DNN3 kernel instead of the weights-stationary one
    uint32_t split_sort_max = 96;  // PG_SPLIT_SORT_MAX: up to this many lists (of 1025 … 8192 items, ~450 K items in all) per call are sorted run by run over the chip (split_sort.hpp; 0 = never)
    uint32_t rank_sort_max = 32;   // PG_RANK_SORT_MAX: up to this many lists per call are sorted by counting ranks (0 = never) ...
    double rank_sort_work = 7e7;   // PG_RANK_SORT_WORK: ... while lists x items^2 stays under this (lists of <= 8192 items; the top-K's final order, one compare per key, takes 1.5 x)
    bool no_r2 = false;            // PG_NO_R2: never refine the int8 screen's suspects on the residual shadow
    double r2_min_factor = 3.0;    // PG_R2_MIN_FACTOR: ... refine once a table's passes average more than this many suspects per answer (x K)
    uint32_t max_rec_scale = 16;   // PG_MAX_REC_SCALE: the 256-query pass's hit-record areas grow up to this many times their default size with a table
                                   // whose batches overflow them (16: 80 B x 123 M records = 9.8 GB per context at K = 5 000); 1 = never (exact scan instead)
    double coalescer_rejoin_us_per_caller = 2.0;   // PG_COALESCER_REJOIN_US: the hold lasts at most 50 + this x n microseconds for a batch of n
    bool coalescer_rejoin = true;  // PG_COALESCER_NO_REJOIN clears it: after a completion a waiting partial batch is held for the callers just answered
    bool no_predict = false;       // PG_NO_PREDICT: never replace the pilot sample by the learned threshold model
    double predict_max_factor = 4.0;   // PG_PREDICT_MAX_FACTOR: a table whose predicted thresholds admit more than this many candidates per answer goes back to the pilot plan
    double predict_sigmas = 4.5;   // PG_PREDICT_SIGMAS: margin of the predicted threshold, in standard deviations of the observed quantile
    uint32_t predict_min_rows = 1u << 22;   // PG_PREDICT_MIN_ROWS: smaller tables are launch-bound either way
    uint32_t screen_early_share_narrow = 512;   // PG_SCREEN_EARLY_SHARE_NARROW: the same for the 8-wave kernels of <= 128 queries
    bool l2_exact = false;                  // PG_L2_EXACT: squared-Euclidean recalls always on the exact scan (A/B runs)
    uint32_t where_compact_max_rows = 8u << 20;   // PG_WHERE_COMPACT_MAX_ROWS: a filter admitting at most this many rows (half of it for <= 4 queries) ...
    uint32_t where_compact_min_ratio = 8;         // PG_WHERE_COMPACT_MIN_RATIO: ... and at most 1/ratio of the table is served from a compact copy of them
    double l2_max_slack = 1.0;              // PG_L2_MAX_SLACK: largest TableDerived::l2_slack the per-BLOCK cutoff is used for (above: the per-row test)
    uint32_t screen_early_share = 604;      // PG_SCREEN_EARLY_SHARE: share (x 1024) of a SIMD's blocks given to its older wave (256-query screen)
    double index_dense_fraction = 0.01;     // PG_INDEX_DENSE_FRACTION: an index recall of nq queries whose (row, query) pairs exceed this x rows x nq^0.6 is served by the table's pass
    uint32_t index_plan_rounds = 2;         // PG_INDEX_PLAN_ROUNDS: expand / rescore / select rounds of an attached index's plan, for the probe and for the scan each
    uint32_t index_skip_batches = 64;       // PG_INDEX_SKIP_BATCHES: after a dense or rounds re-plan, batches of that size band that skip the index plan
    uint32_t coalescer_max_exclude = 0;     // PG_COALESCER_MAX_EXCLUDE: longest list of pg_coalescer_recall_exclude (0..4096; 0: the entry is off), read when a coalescer is created
    uint32_t index_where_cache = 4;         // PG_INDEX_WHERE_CACHE: filtered lists an index keeps per filter (0: built per call, freed after it)
    bool index_route_where = false;         // PG_INDEX_ROUTE_WHERE: pg_recall_topk_where on a table with a current attached index searches it
    uint32_t cf_lds_max_pairs = 6144;           // PG_CF_LDS_MAX_PAIRS: a collaborative-filter request of at most this many (trigger, neighbour) pairs keeps its table in LDS (cf.hip: 12288 slots in 144 KiB, load factor <= 0.5; larger values are cut to that); above, in global memory
    uint32_t fanin_lds_max_cap = 8192;          // PG_FANIN_LDS_MAX_CAP: a fan-in merge of at most this many candidates per request keeps its table in LDS (fanin.hip: 16384 slots of 8 B, load factor <= 0.5; larger values are cut to that); above, in context scratch
    double index_refresh_full_fraction = 0.1;   // PG_INDEX_REFRESH_FULL_FRACTION: pg_index_refresh in auto mode re-assigns every row once the written rows exceed this share of the table
};

}  // namespace pg

struct pg_table {
    // Readers — every enqueue that dereferences the table's pointers, for as long as it reads them — share this lock;
    // pg_table_swap / _upload / _fill take it exclusively and drain the device first.  A request batch (recall, rank,
    // DPP gather: one enqueue) therefore sees ONE table version even when a second context (a coalescer's sibling)
    // enqueues while the table is being swapped.  Lock order: ctx->mu, then the table.
    mutable std::shared_mutex rw;
    // bumped by every exclusive section (upload, fill, swap): a recall job remembers the value it was prepared against, and a
    // re-plan or a patch that finds another one restarts the whole batch on the new rows instead of mixing generations
    mutable std::atomic<uint64_t> generation{0};
    // pg_index_attach: the index that every RecallJob on this table tries first (index.hip).  Written under the exclusive lock
    // with the device drained, read under the shared lock by recall_job_prepare; neither bumps the generation.
    mutable std::atomic<pg_index*> index{nullptr};
    // The write log: every row written by a write that produced a generation in (log_since, generation] lies in
    // one of the log_n disjoint, ascending, non-adjacent ranges [log_lo[i], log_hi[i]).  Written under the exclusive lock the
    // writers hold (TableWrite, table_log_add), read under the shared lock (pg_index_refresh: several indexes of one table at
    // different generations read the same log).  The set only grows between resets.
    static constexpr uint32_t kLogRanges = 64;
    mutable uint64_t log_lo[kLogRanges], log_hi[kLogRanges];
    mutable uint32_t log_n = 0;
    mutable uint64_t log_since = 0;
    float* d = nullptr;          // [rows][dim] fp32 row-major
    uint64_t rows = 0;
    uint32_t dim = 0;
    uint64_t row_offset = 0;     // global row id of local row 0 (sharded tables)
    // a filtered view (pg_table_view_create): the rows of a source table that a WhereClause admits, in row order; recalls
    // report d_row_map[local row] + map_offset — the source's row ids
    uint32_t* d_row_map = nullptr;
    uint64_t map_offset = 0;
    // what is built from the rows and what the plans learn about them (table_state.hpp: lifetimes, update rules, locking)
    mutable pg::TableDerived derived;
    mutable pg::TableLearned learned;
};

// features.hip owns the columns; rank_mlp.hip reads them when it fills item records
struct pg_features {
    uint64_t rows = 0;
    struct Column {
        std::string name;
        int dtype = 0;
        void* d = nullptr;          // [rows] of the column type
        double def = 0.0;           // default for rows outside the store
        uint64_t version = 0;       // pg::next_column_version() at every write of the values (a cache key: never reused)
    };
    std::vector<Column> cols;
};

// materialised item side of an FM + two-tower model (rank_entry.hip builds it, rank_mlp.hip fills it): [rows + 1][kItemRowFloats] fp32
struct pg_item_rows {
    const pg_model* m = nullptr;
    const pg_features* fs = nullptr;
    int32_t cols[16] = {0};
    uint64_t rows = 0;
    float* d = nullptr;
};

struct pg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    std::mutex mu;               // serialises calls on this context
    pg::Scratch scratch[pg::kSlotCount];   // the arena (pg::ScratchSlot); touched only by the scratch_* functions and pg_shutdown
    std::mutex pool_mu;          // guards pipe_free
    std::vector<pg::PipeRun*> pipe_free;     // per-batch status blocks / events of the device-resident pipelines
    std::map<const void*, size_t> dyn_lds;   // kernels whose dynamic-LDS limit was raised on this device
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 0/1 probes, 2/3 rank, 4/5 sort
    std::vector<hipEvent_t> ev_pool;   // per-launch timing events (scan kernel roofline figure)
    uint32_t last_scan_launches = 0;
    bool rank_timing_pending = false;
    pg_stats_t stats{};
    pg::Knobs knobs;
    double last_scan_ms = 0.0;
    uint64_t last_scan_bytes = 0;
    // pinned host staging for small status words
    uint32_t* h_status = nullptr;
    bool timers_off = false;            // (under mu) the call being enqueued records no stage-timer events: TimersScope
};

namespace pg {

typedef std::shared_lock<std::shared_mutex> TableRead;
// shared access to two tables (a recall whose queries are rows of a trigger table): taken in ADDRESS order, the order
// TableWrite(a, b) uses — a reader holding t and waiting for the trigger table against a swap of the two would deadlock
struct TableRead2 {
    TableRead a, b;
    TableRead2(const pg_table* x, const pg_table* y) {
        if (y && y < x) std::swap(x, y);
        a = TableRead(x->rw);
        if (y && y != x) b = TableRead(y->rw);
    }
};
// the write log of a table whose every row may have changed: empty, complete from the generation just produced (caller holds
// the table's lock exclusively and has bumped the generation)
inline void table_log_reset(const pg_table* t) {
    t->log_n = 0;
    t->log_since = t->generation.load(std::memory_order_relaxed);
}
// rows [row0, row0 + n) join the log (merged with the ranges they touch); a 65th range, or more than `full_fraction` of the
// table in the log (the uploading context's "index_refresh_full_fraction"), resets it instead (caller as above)
inline void table_log_add(const pg_table* t, uint64_t row0, uint64_t n, double full_fraction) {
    uint64_t lo = row0, hi = row0 + n;
    uint32_t w = 0, at = 0;
    uint64_t total = 0;
    bool placed = false;
    uint64_t nlo[pg_table::kLogRanges + 1], nhi[pg_table::kLogRanges + 1];
    for (uint32_t i = 0; i < t->log_n; ++i) {
        if (t->log_hi[i] >= lo && t->log_lo[i] <= hi) {          // overlapping or adjacent: absorbed
            lo = std::min(lo, t->log_lo[i]);
            hi = std::max(hi, t->log_hi[i]);
            continue;
        }
        if (!placed && t->log_lo[i] > hi) { at = w++; placed = true; }
        nlo[w] = t->log_lo[i];
        nhi[w] = t->log_hi[i];
        total += nhi[w] - nlo[w];
        ++w;
    }
    if (!placed) at = w++;
    nlo[at] = lo;
    nhi[at] = hi;
    total += hi - lo;
    if (w > pg_table::kLogRanges || (double)total > full_fraction * (double)t->rows) {
        table_log_reset(t);
        return;
    }
    for (uint32_t i = 0; i < w; ++i) { t->log_lo[i] = nlo[i]; t->log_hi[i] = nhi[i]; }
    t->log_n = w;
}
// exclusive access to one or two tables (address order) with nothing in flight on the device.  Every row may change: the write
// log is reset, unless the caller logs the rows it writes itself (keep_log: pg_table_upload, table_log_add)
struct TableWrite {
    std::unique_lock<std::shared_mutex> a, b;
    TableWrite(const pg_table* x, const pg_table* y = nullptr, bool keep_log = false) {
        if (y && y < x) std::swap(x, y);
        a = std::unique_lock<std::shared_mutex>(x->rw);
        x->generation.fetch_add(1, std::memory_order_relaxed);
        if (!keep_log) table_log_reset(x);
        if (y && y != x) {
            b = std::unique_lock<std::shared_mutex>(y->rw);
            y->generation.fetch_add(1, std::memory_order_relaxed);
            if (!keep_log) table_log_reset(y);
        }
    }
};

// ---- recall_plan.hip: a recall whose plans are enqueued without host synchronisation and verified later --------
struct RecallScratch {
    float* qpad;
    float* thr;
    uint32_t* cnt;
    uint32_t* overflow;
    uint64_t* cand[2];
    uint32_t cap;
    // screened scan only
    uint4* qb16;
    float* eps;
    float* thr_screen;
    uint32_t* susp_cnt;      // [kMaxQueries]
    uint32_t* susp;          // [kMaxQueries][cap] suspect rows of the current launch
    float* qscale;           // [kMaxQueries] int8 screen: the queries' scales
    float* thr_ref;          // [kMaxQueries] the thresholds the pilot plan's refinement step raised (verified after the pass)
    uint32_t* q4;            // 4-bit screen: [4][32] int8 queries + [4][4] constants (recall_i4.hip)
    float* pred_ms;          // [kMaxQueries][2] the threshold model's mean and sigma of every query's scores
    // mid-batch screen (recall_i4m.hip): the int8 queries in plain order + the 4-bit bound's constants; the suspects that
    // passed its int8 stage, [kI4mMaxQueries][cap]
    uint32_t* q4m;
    uint32_t* susp2;
    uint32_t* susp2_cnt;     // [kI4mMaxQueries]
    // refinement stage of crowded tables (recall_r2.hip): the queries in sixteen bits + constants; its survivors' counts
    // (their lists share susp2, which holds kMaxQueries lists)
    uint32_t* q16;
    uint32_t* susp2w_cnt;    // [kMaxQueries]
    uint32_t* status;        // [kRecallStatusWords] a job's status words, packed by one kernel for ONE copy to the host
    uint32_t* cnt_seen;      // [kMaxQueries] the candidates each query had collected when the last select kept K of them
};
constexpr uint32_t kRecallStatusWords = 640;
constexpr uint32_t kIndexStatAt = 260;      // an index plan's words in a job's status block ([0, 1 + nq) as every plan's; index.hip, IndexPlanWords in index_shared.hpp)
// A predicate over an integer feature column that restricts a recall's candidates (HologresVectorConf.WhereClause of the
// reference, hologres_vector_recall.go:49-62, in the one shape the device serves: `column OP constant`).  Rows that fail it
// never become candidates — it is applied where candidates are made (exact re-scoring, the exact scan's hit path), so every
// threshold the plans derive is a threshold of the FILTERED top-K and the answers stay exact.
// Its second form serves a compound clause (pg_where, where.hip): dtype = kFilterBits and col the clause's row
// bitmap (bit r & 31 of word r >> 5: row r passes), built once per version of the clause's columns; op and val are unused.
constexpr int kFilterBits = 100;
struct RowFilter {
    const void* col = nullptr;   // [rows] int32 / int64 device column, or the bitmap; nullptr = no filter
    int dtype = 0;               // PG_F_I32, PG_F_I64 or kFilterBits
    int op = 0;                  // pg_where_op: 0 >, 1 >=, 2 <, 3 <=, 4 ==, 5 !=
    long long val = 0;
    long long admitted = -1;     // host side: rows the filter admits when the caller has counted them already (-1: not yet)
};
__host__ __device__ inline bool row_filter_pass(const RowFilter& f, uint32_t row) {
    if (!f.col) return true;
    if (f.dtype == kFilterBits) return (reinterpret_cast<const uint32_t*>(f.col)[row >> 5] >> (row & 31u)) & 1u;
    const long long v = f.dtype == 2 ? reinterpret_cast<const long long*>(f.col)[row] : (long long)reinterpret_cast<const int32_t*>(f.col)[row];
    switch (f.op) {
        case 0: return v > f.val;
        case 1: return v >= f.val;
        case 2: return v < f.val;
        case 3: return v <= f.val;
        case 4: return v == f.val;
        default: return v != f.val;
    }
}

struct IndexServe;   // index_serve.hpp: an attached index's serving counters and switch (outlives the index while a job holds it)
struct RecallJob {
    // set by the caller
    pg_ctx* ctx = nullptr;
    const pg_table* t = nullptr;
    const float* d_queries = nullptr;       // [nq][dim] device
    uint32_t nq = 0, k = 0;
    uint64_t* d_out_rows = nullptr;         // [nq][k] device
    float* d_out_scores = nullptr;          // [nq][k] device
    uint32_t* d_out_count = nullptr;        // [nq] device, optional
    uint32_t* h_status = nullptr;           // pinned host, >= 1 + nq words: [0] overflow flag, [1 + q] valid count of query q
    std::vector<hipEvent_t>* events = nullptr;   // timing events (grown on demand); one job at a time per pool
    bool skip_pilot = false;                // start with the growing-chunk plan (the re-run of a query the pilot failed)
    bool l2 = false;                        // rank by smallest squared Euclidean distance (scores out = distances)
    bool l2_per_row = false;                // ... its screened pass tests every row against its own norm (rows of mixed norms)
    RowFilter filter{};                     // restrict the candidates to the rows that pass (col = nullptr: none)
    uint32_t rows_qualified = 0;            // ... how many rows do (counted in recall_job_prepare)
    bool exact_only = false;                // no statistics, no shadow: the exact scan (the compact table of a selective filter)
    bool no_index = false;                  // never through the table's attached index (its own fallback, the shard group)
    // state (recall_job_*)
    RecallScratch rs{};
    uint32_t* d_count = nullptr;
    uint32_t rows = 0, nblocks = 0;
    bool screen = false;
    bool screen4 = false;                   // the pilot plan's full pass streams the 4-bit shadow (nq <= kI4MaxQueries)
    bool stage2 = false;                    // the int8 screen's suspects pass the two-digit refinement (recall_r2.hip) before the exact re-scoring
    bool screen4m = false;                  // ... through the matrix pipe, suspects thinned on the int8 shadow (kI4MaxQueries < nq <= kI4mMaxQueries)
    int plans[5] = {0, 0, 0, 0, 0};
    bool predict = false;                   // plans[0] takes its first thresholds from the table's threshold model
    bool pred_observe = false;              // the table has a model: this job contributes its observed quantiles
    bool observed = false;                  // ... and the enqueued plan did
    double z_lo = 0.0;
    bool susp_stat = false;                 // the enqueued plan reports its suspect counts with the status words
    bool timers = true;                     // this enqueue recorded its stage-timer events (false: a coalescer batch — recall_job_check reads none)
    bool stat_wide = false;                 // ... and they are the int8 screen's own (no 4-bit stage in front)
    bool refined = false;                   // the enqueued pilot plan raised its thresholds after the first quarter
    int n_plans = 0, next_plan = 0, enqueued_plan = -1;
    uint32_t stride = 1, sample_blocks = 0, k_pilot = 0, perm_mul = 1;
    uint32_t n_ev = 0;
    double scan_ms = 0.0, total_ms = 0.0;
    uint64_t scanned_rows = 0;
    uint64_t scan_bytes = 0;
    uint32_t scan_launches = 0;
    // after a failed check of the pilot plan without overflow: the queries that ended short of K candidates (their
    // sample threshold was too high).  A handful can be re-run one by one instead of re-running the whole batch.
    std::vector<uint32_t> failed;
    uint64_t table_gen = 0;                 // t->generation when the job was prepared (the statistics, shadow and plans are that version's)
    // plans[0] = kIndexPlan: the attached index (read under the shared lock of the enqueue) and its counters (read by the check)
    const pg_index* ix = nullptr;
    std::shared_ptr<IndexServe> ix_serve;
};
constexpr int kIndexPlan = 100;             // the plan id of an attached index's plan (recall_plan.hip's own plans are 0 .. 3)
constexpr size_t kMaxPatchQueries = 8;
// All four: caller holds ctx->mu.  prepare may synchronise once (a table's statistics / shadow on first use).
int recall_job_prepare(RecallJob* j);
int recall_job_enqueue(RecallJob* j);                 // enqueue the next plan + the status copy into h_status
int recall_job_check(RecallJob* j, bool* ok);         // after the stream passed the status copy: did the plan hold?
void recall_job_finish(RecallJob* j);                 // publish timing / counters into ctx
// how a recall job runs besides its table and queries (a default-constructed struct: an inner-product recall of every row)
struct RecallOpts {
    bool skip_pilot = false;                // no pilot plan (a re-run of a failed query)
    bool l2 = false;                        // squared Euclidean, ascending
    const RowFilter* filter = nullptr;      // only the rows the filter admits
    bool exact_only = false;                // the exact plan only
    bool no_index = false;                  // never through an attached index (the index's own fallback)
};
int recall_dev_locked(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k,
                      uint64_t* d_out_rows, float* d_out_scores, uint32_t* out_count, uint32_t* d_out_count,
                      const RecallOpts& o = RecallOpts());
// recall_dev_locked for up to kMaxQueries queries: one job, or for squared Euclidean jobs of at most 128 queries (the screened
// pass serves up to 128; the exact scan runs groups of 64 either way)
int recall_batches_locked(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                          float* d_out_scores, uint32_t* out_count, const RecallOpts& o);
// index.hip: the attached index's plan in front of the table's plans (recall_job_prepare, after the table's plans are made), its
// enqueue-only launches and status copy (recall_job_enqueue) and its verdict (recall_job_check; *ok = false: the table's plans follow)
int index_plan_prepare(RecallJob* j);
int index_plan_enqueue(RecallJob* j, uint32_t status_words);
int index_plan_check(RecallJob* j, bool* ok);
// recall_filter.hip: the checks of pg_recall_topk_where and pg_index_recall_topk_where, in this order, named after `who` (t: the table
// searched); on success *f is the filter.  recall_where_locked: its search, never through an index (caller holds ctx->mu and the
// table's shared lock; device queries and outputs, host counts [nq] or NULL); where_pad_launch: an answer of no admitted row.
int where_check(const char* who, const pg_ctx* ctx, const pg_table* t, const pg_features* fs, int column, int op, long long value,
                int metric, const void* queries, const void* rows, const void* scores, uint32_t nq, uint32_t k, RowFilter* f);
// what a filter is to the caches that key on it (the index's filtered lists): a column of a store, or a compound clause and the
// epoch of its bitmap (where.hip: process-wide, never reused)
struct WhereId {
    const pg_features* fs = nullptr;
    int column = -1;
    const pg_where* w = nullptr;
    uint64_t epoch = 0;
};
// recall_filter.hip: pg_table_view_create behind its checks (caller holds ctx->mu and the table's shared lock; synchronises)
int view_create_locked(const char* who, pg_ctx* ctx, const pg_table* t, const RowFilter& f, pg_table** out_view);
int recall_where_locked(pg_ctx* ctx, const pg_table* t, RowFilter f, int metric, const float* d_q, uint32_t nq, uint32_t k,
                        uint64_t* d_rows, float* d_sc, uint32_t* out_count);
int where_pad_launch(pg_ctx* ctx, uint64_t* d_rows, float* d_sc, size_t n, bool l2);
// where.hip: a compound clause for a search outside that file (pg_recall_topk_exclude).  where_clause_check: the checks of
// pg_recall_topk_where_ex in its order (no lock needed); where_clause_bind: the filter, its identity and the reference that keeps
// its bitmap alive until the caller's stream has synchronised (caller holds ctx->mu and the table's shared lock).
struct WhereServe {
    RowFilter f{};
    WhereId id{};
    std::shared_ptr<void> hold;
};
int where_clause_check(const char* who, const pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, int metric,
                       const void* queries, const void* rows, const void* scores, uint32_t nq, uint32_t k);
int where_clause_bind(const char* who, pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, WhereServe* out);
// where.hip: the clause's BITMAP over `rows` rows of `fs`, a one-comparison clause's too (coldstart.hip: the pool of a
// ColdStartRecall): its columns resolved with where_resolve's rules, the bitmap built or found current; out->f.admitted is the
// rows it admits, out->id.epoch its epoch.  Caller holds ctx->mu; a build synchronises.
int where_bits_bind(const char* who, pg_ctx* ctx, const pg_where* w, const pg_features* fs, uint64_t rows, WhereServe* out);
// exclude.hip: pg_exclude_compact_dev behind its checks (caller holds ctx->mu; enqueues one kernel, nothing synchronises)
constexpr uint32_t kMaxExclude = 4096;      // ids in one request's list
int exclude_compact_locked(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t k_in,
                           const uint64_t* d_excl_rows, const uint32_t* d_excl_offsets, uint32_t k_out, float pad_score,
                           uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count);
// fanin.hip: the merge of n_src recall answers per request (one launch, no synchronisation; arguments as pg_fanin_merge_dev, checked by the caller)
int fanin_merge_locked(pg_ctx* ctx, const pg_fanin_source* src, uint32_t n_src, uint32_t nq, uint64_t* d_out_rows, double* d_out_score,
                       uint8_t* d_out_source, double* d_out_recall_scores, uint32_t* d_out_source_mask, uint32_t* d_out_count);
// index.hip: the attached index pg_recall_topk_where searches ("index_route_where" set and the index current), or NULL; the
// filtered search itself (a stale, non-finite, dense or overflowing batch: recall_where_locked)
pg_index* index_route_where(const pg_ctx* ctx, const pg_table* t);
int index_where_locked(pg_ctx* ctx, pg_index* ix, const WhereId& id, const RowFilter& f, bool l2, const float* d_q,
                       uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc, uint32_t* h_counts);
const pg_table* index_table(const pg_index* ix);
// index_assign.hip: the matrix-pipe assignment of pg_index_refresh's full path (dim 64 / 128).  The split bf16
// screen over all lists with the survivors confirmed by the rule's chain: out[r] = the rule's list of row r, except for the
// rows the screen could not settle (more survivors than slots, a row outside the range the bound is proven for), whose ids are
// appended to wide[*wide_n ...] in no particular order.  *flag |= 1 for a non-finite row element.  ws: assign_screen_ws_bytes()
// of device memory.  Returns PG_ERR_UNSUPPORTED (nothing enqueued beyond the workspace's preparation, which synchronises) when
// a centroid lies outside that range: the caller assigns with the fp32 kernel.
size_t assign_screen_ws_bytes(uint32_t nl, uint32_t dim);
int assign_screen_launch(pg_ctx* ctx, uint32_t dim, const float* X, uint64_t n, const float* C, uint32_t nl, void* ws, uint32_t* out,
                         uint32_t* wide, uint32_t* wide_n, uint32_t* flag);
// features.hip: a process-wide counter, so a column's version never repeats (not even for a store reallocated at one address)
uint64_t next_column_version();
// re-run the failed queries of `j` (at most kMaxPatchQueries) one by one, synchronously, writing into their slices of
// the job's outputs and their valid counts into counts[q]; caller holds ctx->mu
int recall_patch_failed_locked(RecallJob* j, uint32_t* counts);
// Stage timers (HIP events around the recall plan, its scan launches and the rank stage: pg_stats' last_*_ms, pg_last_scan_kernel_ms)
// cost ~6 us of idle queue per record — 40-60 us of a 1.3-1.8 ms small-batch step.  A caller that reads none of them (the coalescer:
// its statistics are enqueue -> completion times) switches them off for the calls it enqueues; caller holds ctx->mu.
struct TimersScope {
    pg_ctx* ctx;
    bool prev;
    TimersScope(pg_ctx* c, bool timers) : ctx(c), prev(c->timers_off) { c->timers_off = prev || !timers; }      // (only ever off: pg_set_option "stage_timers" 0 stays in force)
    ~TimersScope() { ctx->timers_off = prev; }
};
int recall_scratch(pg_ctx* ctx, uint32_t dim, uint32_t k, RecallScratch* rs);
int launch_select(pg_ctx* ctx, uint32_t nq, const uint64_t* in, uint64_t* out, uint32_t* cnt, float* thr,
                  uint32_t cap, uint32_t k, int thr_only = 0, uint32_t* cnt_seen = nullptr);
int final_launch(pg_ctx* ctx, const uint64_t* cand, const uint32_t* cnt, uint32_t cap, uint32_t nq, uint32_t k,
                 uint64_t row_offset, uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count);
// recall_table.hip: the lazy builds of pg_table::derived (each takes g_table_state_mu itself: never call one with it held)
int ensure_table_stats(pg_ctx* ctx, const pg_table* t);
int ensure_table_nx(pg_ctx* ctx, const pg_table* t);
// what the plans learnt about a table, as a copy taken under g_table_state_mu: how pg_table::learned is read (table_state.hpp)
inline TableLearned table_learned(const pg_table* t) {
    std::lock_guard<std::mutex> g(g_table_state_mu);
    return t->learned;
}
// recall.hip's exact re-scoring (rescore_kernel) over per-query suspect lists susp[q * scap + i] of local rows, appending the keys of
// rows whose score reaches thr[q] to cand[q * cap + ...]; the squared-Euclidean |q|^2 chain and the final sign flip — for the plans
// (recall_plan.hip) and index_search.hip.  blocks = 0: the table pass's own grid; rows that fail `filter` are no candidates
int rescore_launch(pg_ctx* ctx, uint32_t dim, bool l2, const float* tab, const float* d_queries, const float* thr, const uint32_t* susp,
                   const uint32_t* susp_cnt, uint32_t scap, uint32_t* cnt, uint64_t* cand, uint32_t* overflow, uint32_t cap, uint32_t nq,
                   uint32_t n_rows, const float* nx, const float* nqv, uint32_t blocks, const RowFilter& filter = RowFilter());
int query_norm2_launch(pg_ctx* ctx, const float* d_queries, uint32_t nq, uint32_t dim, float* d_out);
int negate_launch(pg_ctx* ctx, float* d_v, uint64_t n);
// recall_i4.hip (caller holds ctx->mu)
constexpr uint32_t kI4MaxQueries = 4;
int ensure_table_i4(pg_ctx* ctx, const pg_table* t);
int screen4_prep_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs);
int screen4_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, uint32_t nq, uint32_t row_begin, uint32_t row_end,
                   uint32_t cap4, const float* l2_nqv = nullptr);
uint32_t screen4_rescore_blocks();
// recall_i4m.hip (caller holds ctx->mu): the same shadow through the int8 matrix pipe for 5 .. kI4mMaxQueries queries
constexpr uint32_t kI4mMaxQueries = 64;
constexpr uint32_t kQ4mWords = kI4mMaxQueries * 32 + kI4mMaxQueries * 4 + 4;
int screen4m_prep_launch(pg_ctx* ctx, const RecallScratch& rs, uint32_t nq);
// recall_r2.hip (caller holds ctx->mu)
int ensure_table_r2(pg_ctx* ctx, const pg_table* t);
int rescreen16_prep_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, uint32_t nq);
int rescreen16_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, uint32_t nq);
int screen4m_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, uint32_t nq, uint32_t row_begin, uint32_t row_end,
                    uint32_t cap1, bool susp2_clean = false);
int topk_merge_strided_locked(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t nlists,
                              uint32_t per_list, size_t row_ls, size_t row_qs, size_t sc_ls, size_t sc_qs, uint32_t k,
                              uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count);
int topk_merge_locked(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t nlists,
                      uint32_t per_list, int list_major, uint32_t k, uint64_t* d_out_rows, float* d_out_scores,
                      uint32_t* d_out_count);

// ---- stage launchers shared with pipeline.hip (caller holds ctx->mu; nothing synchronises) -------------------
// head o of a multi-head model writes d_out + o * out_stride (out_stride = 0: n_items)
int rank_dnn3_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user,
                         const uint32_t* d_cand, const uint32_t* d_off, uint32_t n_req, uint32_t n_items,
                         float* d_out, size_t out_stride = 0);
int fm2t_user_embedding_locked(pg_ctx* ctx, const pg_model* m, const float* d_user, uint32_t n_req, float* d_out);
// candidates as per-item field ids (d_ifids), or as rows of item records (ir, d_cand)
int rank_fm2t_dev_locked(pg_ctx* ctx, const pg_model* m, const float* d_user, const int32_t* d_ufids, const int32_t* d_ifids,
                         const uint32_t* d_off, uint32_t n_req, uint32_t n_items, float* d_out, const pg_item_rows* ir = nullptr,
                         const uint32_t* d_cand = nullptr);
int item_rows_fill_locked(pg_ctx* ctx, pg_item_rows* ir, uint64_t row0, uint64_t nrows);
int rank_fm2t_irows_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_item_rows* ir, const float* d_user, const int32_t* d_ufids,
                               const uint32_t* d_cand, const uint32_t* d_off, uint32_t n_req, uint32_t n_items, float* d_out);
int rank_fm2t_rows_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                              const float* d_user, const int32_t* d_ufids, const uint32_t* d_cand, const uint32_t* d_off,
                              uint32_t n_req, uint32_t n_items, float* d_out);
// d_err: device flags, OR-ed with 1 where an item divides by zero; item i reports into d_err[i / items_per_flag]
// (items_per_flag = 0: one flag for the call)
int expr_eval_enqueue_locked(pg_ctx* ctx, const pg_expr* e, const double* d_vars, uint32_t n_items, double* d_out,
                             uint32_t* d_err, uint32_t items_per_flag);
void set_expr_arith_error(const pg_expr* e);
// RankConfig.ScoreRewrite attached to a RankScore expression (pg_expr_set_score_rewrites; expr.hip)
constexpr int kMaxRewrites = 8;
// Holders of a compiled RankScore: everything that keeps a variable binding made from it (recommend_bind_vars: coalescers for their
// lifetime, tickets until they are ended, pg_fuse_scores_dev for the call).  pg_expr_set_score_rewrites refuses while there is
// one — the bindings are sized for the rewrites attached at that moment.
void expr_hold(const pg_expr* e);
void expr_release(const pg_expr* e);
struct ExprHold {
    const pg_expr* e = nullptr;
    ExprHold() = default;
    ExprHold(const ExprHold&) = delete;
    ExprHold& operator=(const ExprHold&) = delete;
    void take(const pg_expr* x) {
        if (e) expr_release(e);
        e = x;
        if (e) expr_hold(e);
    }
    ~ExprHold() { if (e) expr_release(e); }
};
int expr_num_rewrites(const pg_expr* e);
const char* expr_rewrite_source(const pg_expr* e, int r);
int expr_rewrite_num_vars(const pg_expr* e, int r);
const char* expr_rewrite_var_name(const pg_expr* e, int r, int i);
int expr_rewrite_eval_enqueue_locked(pg_ctx* ctx, const pg_expr* e, int r, const double* d_vars, uint32_t n_items, double* d_out,
                                     uint32_t* d_err, uint32_t items_per_flag);
int table_gather_locked(pg_ctx* ctx, const pg_table* t, const uint32_t* d_rows, uint32_t n, float* d_out);
int dpp_run_locked(pg_ctx* ctx, const float* d_emb32, const double* d_hook, const double* d_rel, uint32_t R, uint32_t n,
                   uint32_t d, uint32_t hook_dim, double alpha, uint32_t topn, uint32_t window, int normalize,
                   int ensure_pos, int has_table, uint32_t* d_out, uint32_t* d_out_count, double* d_L_out = nullptr);
int sort_dev_locked(pg_ctx* ctx, const double* d_scores, const uint32_t* d_seg, uint32_t n_seg, uint32_t n_items,
                    uint32_t max_seg, int desc, uint32_t* d_out);

void pipe_pool_destroy(pg_ctx* ctx);      // pipeline.hip
// the arena (api.cpp): at least `bytes` of the slot; growing it synchronises the stream, frees and reallocates.  A failed
// allocation is a device error — or, when `soft`, PG_ERR_NOMEM with the sticky HIP error cleared and the slot left empty
int scratch_reserve(pg_ctx* ctx, ScratchSlot slot, size_t bytes, void** out, bool soft = false);
const void* scratch_peek(const pg_ctx* ctx, ScratchSlot slot);     // what the slot holds now (nullptr: never reserved), for diagnostics
// reserve a slot for the layout `lay(Carve&)` states: run once to measure, once more over the reserved buffer
template <class Layout>
int scratch_carve(pg_ctx* ctx, ScratchSlot slot, Layout&& lay, bool soft = false) {
    Carve c;
    lay(c);
    void* buf;
    const int rc = scratch_reserve(ctx, slot, c.total(), &buf, soft);
    if (rc == PG_OK) lay(c = Carve{(char*)buf});
    return rc;
}
// the checks of the pg_recall_topk* and pg_index_recall_topk* entry points, in this order, named after the entry point `who`;
// `over` is the table or index searched (its dim)
template <class T>
int recall_check(const char* who, const pg_ctx* ctx, const T* over, const void* queries, const void* rows, const void* scores, uint32_t nq,
                 uint32_t k, bool l2) {
    PG_REQUIRE(ctx && over && queries && rows && scores, "%s: NULL argument", who);
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    PG_REQUIRE(l2 || over->dim <= 128 || nq <= 32, "%s: dim %u supports at most 32 queries per call", who, over->dim);
    if (k < 1 || k > 16384) {
        set_error("%s: k=%u unsupported (1..16384)", who, k);
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}
// a recall into host outputs through the staging slot: the queries copied from the host — or, with `queries` NULL, brought by
// fill(d_queries) —, run(d_queries, d_rows, d_scores) on the device, then the rows and scores copied out; caller holds ctx->mu
template <class Run>
int recall_staged(pg_ctx* ctx, uint32_t dim, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, Run&& run,
                  const std::function<int(float*)>& fill = nullptr) {
    float *d_q, *d_sc; uint64_t* d_rows; int rc;
    if ((rc = scratch_carve(ctx, kSlotStaging, [&](Carve& c) {
            d_q = c.take<float>((size_t)nq * dim);
            d_rows = c.take<uint64_t>((size_t)nq * k);
            d_sc = c.take<float>((size_t)nq * k);
        }))) return rc;
    if (queries) PG_HIP(hipMemcpyAsync(d_q, queries, (size_t)nq * dim * 4, hipMemcpyHostToDevice, ctx->stream));
    else if ((rc = fill(d_q))) return rc;
    if ((rc = run(d_q, d_rows, d_sc))) return rc;
    PG_HIP(hipMemcpyAsync(out_rows, d_rows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(out_scores, d_sc, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}
// raise a kernel's dynamic-LDS limit once per context (the attribute is per device: a process may hold
// contexts on several GPUs); caller holds ctx->mu
int ensure_dyn_lds(pg_ctx* ctx, const void* kernel, size_t bytes);
// features.hip: gather of integer feature columns, caller holds ctx->mu
int features_gather_i32_locked(pg_ctx* ctx, const pg_features* fs, const int32_t* col_idx, uint32_t n_cols,
                               const uint32_t* d_rows, uint32_t n, int32_t* d_out, const char* who);
}
