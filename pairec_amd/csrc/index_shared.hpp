// index_shared.hpp — what more than one of index.hip, index_build.hip, index_search.hip and index_where.hip needs and no file
// outside them does (what other files call is declared in common.hpp; the host-side rules are index_serve.hpp's).
#pragma once
#include "common.hpp"
#include "index_serve.hpp"

#include <list>

namespace pg {
// The lists of an index restricted to the rows a filter admits: list L holds perm[off[L], off[L + 1]), the
// index's rows of L that pass, in the same (ascending source) order.  One allocation, freed with the last reference: a call that
// searches an entry holds it until its stream has synchronised, so an eviction by another context never frees it under a search.
struct WhereLists {
    WhereKey key{};
    void* d = nullptr;
    uint32_t* off = nullptr;             // [n_lists + 1]
    uint32_t* perm = nullptr;            // [admitted]
    uint64_t admitted = 0;
    size_t bytes = 0;                    // admitted x 4 + (n_lists + 1) x 4 (the offsets padded to 256 B)
    ~WhereLists() { if (d) (void)hipFree(d); }
};

// An index's device arrays: two allocations, `perm` and `small` — the latter carved into off | cent | cnorm | rad.  Allocated,
// carved and released by index_build.hip alone (index_arrays_alloc / index_arrays_free: the layout is written there, once);
// a refresh builds a second set and exchanges the two.
struct IndexArrays {
    uint32_t* perm = nullptr;     // [rows] source rows, list by list
    void* small = nullptr;        // the allocation behind off / cent / cnorm / rad
    uint32_t* off = nullptr;      // [n_lists + 1] list offsets into perm
    float* cent = nullptr;        // [n_lists][dim] centroids
    float* cnorm = nullptr;       // [n_lists] ||c_L||, rounded up
    float* rad = nullptr;         // [n_lists] r_L, rounded up
};
}  // namespace pg

struct pg_index {
    const pg_table* t = nullptr;
    uint64_t gen = 0;
    uint64_t rows = 0;
    uint32_t dim = 0, n_lists = 0;
    bool nonfinite = false;
    pg::IndexArrays a;            // (exchanged by pg_index_refresh under the table's exclusive lock)
    std::mutex mu;                // guards st
    pg_index_stats_t st{};        // the synchronous pg_index_recall_topk* calls (the attached plans count in serve)
    std::shared_ptr<pg::IndexServe> serve = std::make_shared<pg::IndexServe>();
    // filtered lists: at most "index_where_cache" entries, most recently used first.  where_mu is taken after
    // ctx->mu and the table's shared lock; it also guards where_st.
    std::mutex where_mu;
    pg::WhereCache<pg::WhereLists> where_cache;
    pg_index_where_stats_t where_st{};
    // pg_index_refresh: one refresh of an index at a time (taken after ctx->mu, before the table's lock); the
    // counters are guarded by mu
    std::mutex refresh_mu;
    pg_index_refresh_stats_t rst{};
};

namespace pg {

constexpr uint32_t kSlices = 256;        // list slices of the count / expand kernels (per query)

// the verdict of an index plan, written by the device (index_plan_kernel) and read by every later launch of the plan, then
// copied into the job's status words at kIndexStatAt
struct IndexPlanWords {
    uint32_t flags;                      // kPlanNonfinite | kPlanDense | kPlanRounds: the table's plans serve the batch
    uint32_t need[2];                    // rounds the probe (0) and the scan (1) take
    uint32_t max_probe;                  // the most rows one query's probe scores
    unsigned long long pairs[2];         // (row, query) pairs of the probe and the scan
    unsigned long long union_rows;       // rows of the lists live for some query (union_kernel)
    unsigned long long max_scan;         // the most rows one query's scan scores
};
static_assert(sizeof(IndexPlanWords) == 48, "12 status words");

// the smallest float >= v
__device__ __forceinline__ float round_up_f(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, __builtin_inff());
    return f;
}

// device allocation that reports failure as PG_ERR_NOMEM (and clears the runtime's last error)
inline int dalloc(void** p, size_t bytes) {
    if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return PG_ERR_NOMEM;
    }
    return PG_OK;
}
// ... into a list that free_all releases
inline int dalloc(void** p, size_t bytes, std::vector<void*>& owned) {
    const int rc = dalloc(p, bytes);
    if (rc == PG_OK) owned.push_back(*p);
    return rc;
}

inline void free_all(std::vector<void*>& owned) {
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
}

// kSlotIndexSearch of one batch (NOMEM instead of a device error when it cannot grow): U [nq][nl] | qn [nq] f64 | nqv [nq] | Bkey [nq] | probe rows [nq] | counts [nq] | the plan's words [16] |
//          slice counts [nq][kSlices] | scan threshold [nq]
struct SearchBufs {
    float* U;
    double* qn;
    float* nqv;
    uint32_t *Bkey, *probe, *dcount;
    IndexPlanWords* pw;
    uint32_t* cntg;
    float* thr_scan;                     // the probe's K-th scores, frozen for the scan's list selection
};

// The lists a search walks: the index's own, or a filter's — the same sequence over either.  rows: the rows
// the lists hold (the probe covers min(K, rows) of them); dense_rows: the rows the dense rule weighs the batch's pairs against.
struct SearchLists {
    const uint32_t* perm;
    const uint32_t* off;
    uint64_t rows;
    double dense_rows;
};

// index_search.hip (both described there)
int search_bufs(pg_ctx* ctx, uint32_t nq, uint32_t nl, SearchBufs* b);
int index_search(pg_ctx* ctx, const pg_index* ix, const SearchLists& li, const float* d_q, uint32_t nq, uint32_t k, bool l2, RecallScratch& rs,
                 const SearchBufs& sb, uint64_t* d_rows, float* d_sc, uint32_t* d_count, uint32_t budget, IndexPlanWords* h_pw);
// index_where.hip: the filter's lists from the index's cache, or built; caller holds ctx->mu and the table's shared lock
int where_lists_get(pg_ctx* ctx, pg_index* ix, const WhereId& id, const RowFilter& f, std::shared_ptr<WhereLists>* out);

}  // namespace pg
