// index_serve.hpp — the host-side rules of the exact IVF index, each written once.  No HIP and nothing
// that needs it: what the device measured comes in as arguments, so every rule can be checked on the CPU with hand-made
// values (tests/index_serve_check.cpp).  The index's units (index.hip, index_build.hip, index_where.hip) call these and keep
// no second copy.
//
// The rules, once:
// * Build.  n_lists 0 = round(4 sqrt(rows)), clamped to kMaxLists, to rows / 64 and to at least 1; train_rows 0 = min(rows,
//   64 n_lists), clamped to [n_lists, rows] (rows first); iters 0 = 8.
// * Pre-search.  Before anything is launched a batch is `stale` (the table's generation is not the index's), else `nonfinite`
//   (the table holds a non-finite value), else `l2_dim` (squared Euclidean at a dim other than 64 / 128: the search has no
//   kernel for it) — in that order.  The synchronous searches answer these by their fallback pass, counted as stale,
//   nonfinite and dense; an attached plan is not tried.
// * Bands.  Batch sizes 1, 2-8, 9-32, 33-64, 65-256.  A band's switch holds the batches that still skip the index plan; every
//   batch of the band takes one off until it is 0.
// * A finished plan (its flags and overflow word have arrived).  non-finite, else dense (also when rounds is set with it),
//   else rounds, else overflow, else held.  Dense and rounds arm the band's switch with index_skip_batches (at most
//   0x7FFFFFFF); only a held plan counts its pairs, live rows and longest scan.
// * pg_index_stats = the synchronous calls' counters + the plans' (a rounds re-plan has no field there).
// * Refresh.  mode 2 is incremental, refused when the table's write log does not reach back to the index's generation; mode 1
//   is full; so is a forced refresh of a current index; mode 0 is incremental when the log covers and holds at most
//   full_fraction x rows, else full.
// * The filtered lists' cache.  Most recently used first.  A call trims to the CALLING context's capacity, then looks its key
//   up (a hit moves to the front), else builds; what it built is kept only at a capacity above 0, and the cache trimmed again.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <list>
#include <memory>

#include "../../include/pairec_gpu.h"

namespace pg {

// ---- build ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxLists = 65536;

struct IndexBuildShape {
    uint32_t n_lists;
    uint64_t train_rows;                 // the k-means sample
    uint32_t iters;
};
inline IndexBuildShape index_build_shape(uint64_t rows, const pg_index_params& p) {
    uint32_t nl = p.n_lists;
    if (nl == 0) nl = (uint32_t)std::llround(4.0 * std::sqrt((double)rows));
    if (nl > kMaxLists) nl = kMaxLists;
    if (nl > rows / 64) nl = (uint32_t)(rows / 64);
    if (nl < 1) nl = 1;
    uint64_t ns = p.train_rows ? p.train_rows : std::min<uint64_t>(rows, 64ull * nl);
    if (ns > rows) ns = rows;
    if (ns < nl) ns = nl;
    return IndexBuildShape{nl, ns, p.iters ? p.iters : 8u};
}

// ---- before a search -----------------------------------------------------------------------------------------------
enum class IndexPre { search, stale, nonfinite, l2_dim };
inline IndexPre index_pre_search(uint64_t table_gen, uint64_t index_gen, bool table_nonfinite, bool l2, uint32_t dim) {
    if (table_gen != index_gen) return IndexPre::stale;
    if (table_nonfinite) return IndexPre::nonfinite;
    if (l2 && dim != 64 && dim != 128) return IndexPre::l2_dim;
    return IndexPre::search;
}
// the pg_index_stats counter of the fallback a synchronous search takes then (null: it searches)
inline uint64_t pg_index_stats_t::*index_pre_fallback(IndexPre v) {
    switch (v) {
        case IndexPre::stale: return &pg_index_stats_t::fallback_stale;
        case IndexPre::nonfinite: return &pg_index_stats_t::fallback_nonfinite;
        case IndexPre::l2_dim: return &pg_index_stats_t::fallback_dense;   // (the fallback pass answers with its own error)
        case IndexPre::search: break;
    }
    return nullptr;
}

// ---- serving through an attached index -----------------------------------------------------------------------------
// an attached index's serving counters and its switch, shared with the jobs that tried it (a job's check may come after a
// detach and destroy: the jobs keep this alive, not the index)
constexpr int kBands = 5;                  // batch sizes 1, 2-8, 9-32, 33-64, 65-256
struct IndexServe {
    std::atomic<uint64_t> plans{0}, plans_held{0}, queries_held{0};
    std::atomic<uint64_t> replan_dense{0}, replan_rounds{0}, replan_overflow{0}, replan_nonfinite{0};
    std::atomic<uint64_t> skipped_stale{0}, skipped_switch{0};
    std::atomic<uint64_t> queries{0}, pairs{0}, rows_live{0}, max_scan{0};
    std::atomic<int32_t> skip[kBands] = {};   // batches of the band that skip the index plan before it is tried again
};

inline int band_of(uint32_t nq) { return nq <= 1 ? 0 : nq <= 8 ? 1 : nq <= 32 ? 2 : nq <= 64 ? 3 : 4; }

// one batch of nq queries against its band's switch: true when it skips the index plan (one taken off the countdown)
inline bool serve_take_skip(IndexServe& sv, uint32_t nq) {
    std::atomic<int32_t>& sw = sv.skip[band_of(nq)];
    int32_t left = sw.load(std::memory_order_relaxed);
    while (left > 0 && !sw.compare_exchange_weak(left, left - 1, std::memory_order_relaxed)) {}
    if (left <= 0) return false;
    sv.skipped_switch++;
    return true;
}

// the verdict the device writes into an index plan's words (IndexPlanWords::flags): the table's plans serve the batch
constexpr uint32_t kPlanNonfinite = 1u, kPlanDense = 2u, kPlanRounds = 4u;

enum class PlanVerdict { held, nonfinite, dense, rounds, overflow };
inline PlanVerdict plan_verdict(uint32_t flags, uint32_t overflow_word) {
    if (flags & kPlanNonfinite) return PlanVerdict::nonfinite;
    if (flags & kPlanDense) return PlanVerdict::dense;
    if (flags & kPlanRounds) return PlanVerdict::rounds;
    return overflow_word != 0 ? PlanVerdict::overflow : PlanVerdict::held;
}
inline bool plan_arms_switch(PlanVerdict v) { return v == PlanVerdict::dense || v == PlanVerdict::rounds; }
inline int32_t plan_switch_batches(uint32_t index_skip_batches) { return (int32_t)std::min<uint32_t>(index_skip_batches, 0x7FFFFFFFu); }

// a finished plan of nq queries enters the counters; pairs, union_rows and max_scan are its words' (counted when it held)
inline PlanVerdict serve_plan_done(IndexServe& sv, uint32_t nq, uint32_t flags, uint32_t overflow_word, uint32_t index_skip_batches,
                                   uint64_t pairs, uint64_t union_rows, uint64_t max_scan) {
    const PlanVerdict v = plan_verdict(flags, overflow_word);
    sv.plans++;
    sv.queries += nq;
    switch (v) {
        case PlanVerdict::nonfinite: sv.replan_nonfinite++; break;
        case PlanVerdict::dense: sv.replan_dense++; break;
        case PlanVerdict::rounds: sv.replan_rounds++; break;
        case PlanVerdict::overflow: sv.replan_overflow++; break;
        case PlanVerdict::held: {
            sv.plans_held++;
            sv.queries_held += nq;
            sv.pairs += pairs;
            sv.rows_live += union_rows;
            uint64_t m = sv.max_scan.load(std::memory_order_relaxed);
            while (max_scan > m && !sv.max_scan.compare_exchange_weak(m, max_scan, std::memory_order_relaxed)) {}
            break;
        }
    }
    if (plan_arms_switch(v)) sv.skip[band_of(nq)].store(plan_switch_batches(index_skip_batches), std::memory_order_relaxed);
    return v;
}

// pg_index_stats: + the batches that tried the attached plan (`rounds` re-plans have no field of their own here)
inline void serve_fold_stats(const IndexServe& sv, pg_index_stats_t* out) {
    const uint64_t pairs = sv.pairs.load();
    out->calls += sv.plans.load();
    out->queries += sv.queries.load();
    out->rows_scored += pairs;
    out->pairs_scored += pairs;
    out->rows_live += sv.rows_live.load();
    out->max_query_scan_rows = std::max<uint64_t>(out->max_query_scan_rows, sv.max_scan.load());
    out->fallback_dense += sv.replan_dense.load();
    out->fallback_nonfinite += sv.replan_nonfinite.load();
    out->fallback_overflow += sv.replan_overflow.load();
}

// ---- refresh -------------------------------------------------------------------------------------------------------
// what a refresh that is not a no-op does.  covered: the table's write log holds every write since the index's generation;
// logged: the rows in it; current: the table's generation is the index's (the refresh was forced)
enum class RefreshPlan { refused, full, incremental };
inline RefreshPlan refresh_plan(int mode, bool covered, uint64_t logged, uint64_t rows, double full_fraction, bool current) {
    if (mode == 2) return covered ? RefreshPlan::incremental : RefreshPlan::refused;
    if (mode == 1 || current) return RefreshPlan::full;
    return covered && (double)logged <= full_fraction * (double)rows ? RefreshPlan::incremental : RefreshPlan::full;
}

// ---- the filtered lists' cache ----------------------------------------------------------------------
struct WhereKey {
    const pg_features* fs;
    int column;
    uint64_t version;                    // the column's (process-wide counter: a rewritten or reallocated column never matches)
    int op;
    long long value;
    uint64_t gen;                        // the index's table generation
    // a compound clause: its identity and its bitmap's epoch (column -1; version, op and value 0) — a bitmap
    // rebuilt after a column changed has a new epoch, and no two builds in a process share one
    const pg_where* w;
    uint64_t epoch;
    bool operator==(const WhereKey& o) const {
        return fs == o.fs && column == o.column && version == o.version && op == o.op && value == o.value && gen == o.gen && w == o.w &&
               epoch == o.epoch;
    }
};

// Entry: anything with a `WhereKey key` and a `size_t bytes`
template <class Entry>
using WhereCache = std::list<std::shared_ptr<Entry>>;

template <class Entry>
void where_cache_trim(WhereCache<Entry>& c, pg_index_where_stats_t& st, uint32_t cap) {
    while (c.size() > cap) {
        st.evictions++;
        st.bytes -= c.back()->bytes;
        c.pop_back();                    // (a search that still holds the entry keeps it alive)
    }
    st.entries = c.size();
}

// the entry of `key`: from the cache, or from build(out) (an int status, 0 = built: returned as it is otherwise)
template <class Entry, class Build>
int where_cache_get(WhereCache<Entry>& c, pg_index_where_stats_t& st, uint32_t cap, const WhereKey& key, std::shared_ptr<Entry>* out,
                    Build&& build) {
    where_cache_trim(c, st, cap);        // (to the calling context's capacity: at 0 every call builds)
    for (auto it = c.begin(); it != c.end(); ++it) {
        if (!((*it)->key == key)) continue;
        c.splice(c.begin(), c, it);
        st.hits++;
        *out = c.front();
        return 0;
    }
    if (const int rc = build(out)) return rc;
    (*out)->key = key;
    st.builds++;
    if (cap) {
        c.push_front(*out);
        st.bytes += (*out)->bytes;
    }
    where_cache_trim(c, st, cap);
    return 0;
}

template <class Entry>
void where_cache_clear(WhereCache<Entry>& c, pg_index_where_stats_t& st) {
    c.clear();
    st.entries = 0;
    st.bytes = 0;
}

}  // namespace pg
