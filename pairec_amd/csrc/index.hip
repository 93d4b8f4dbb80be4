// index.hip — an exact IVF-partitioned index over a table: what ties its units together.
//   index_build.hip    the k-means build, pg_index_refresh, destroy and read; the layout of an index's device arrays
//   index_search.hip   the bound / probe / scan search (index_search) with its device-written plan words
//   index_where.hip    a filter's lists over the index and their cache
//   index_serve.hpp    the host-side rules, without HIP: pre-search verdicts, bands and switches, a finished plan's verdict, ...
//   index_shared.hpp   pg_index and what two of the units need
//
// One launch sequence (index_search) serves both callers here.  They differ only in their round policy:
//   pg_index_recall_topk*   the host reads the words after each stage, falls back to the table's pass on a flag, and runs exactly
//                           the rounds counted (no budget)
//   an attached index       (pg_index_attach) a RecallJob plan that is only enqueued: index_plan_rounds rounds per
//                           stage, rounds past the verdict's do nothing; recall_job_check reads the words with the job's status
//                           words and moves to the table's own plans when a flag is set
#include "index_shared.hpp"

#include <cmath>

namespace pg {
namespace {

// the dense rule of a filter's lists: the filtered pass costs about as much as the table's pass (rows) or, when
// it gathers a compact copy, this many table-pass rows per admitted row (profiles/index_where.json: the breakevens at 0.1 % and
// 1 % admitted put it at ~140 and ~80)
constexpr double kWhereGatherWeight = 150.0;

// the status block of an index plan (<<<1, kMaxQueries>>>): [0] the re-scoring's overflow flag, [1 + q] valid counts (as every
// plan's), [kIndexStatAt, + 12) the plan's words
__global__ void index_status_kernel(const uint32_t* __restrict__ overflow, uint32_t nq, const IndexPlanWords* __restrict__ pw,
                                    uint32_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    out[1 + t] = t < nq ? overflow[1 + t] : 0u;
    if (t < sizeof(IndexPlanWords) / 4) out[kIndexStatAt + t] = reinterpret_cast<const uint32_t*>(pw)[t];
    if (t == 0) out[0] = overflow[0];
}

SearchLists own_lists(const pg_index* ix) { return SearchLists{ix->a.perm, ix->a.off, ix->rows, (double)ix->rows}; }

int table_pass_locked(pg_ctx* ctx, const pg_table* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc,
                      uint32_t* h_counts, bool l2) {
    RecallOpts o;
    o.l2 = l2;
    o.no_index = true;                   // (never through an attached index: this is the index's own fallback)
    return recall_batches_locked(ctx, t, d_q, nq, k, d_rows, d_sc, h_counts, o);
}

// One batch, synchronously (caller holds ctx->mu and the table's shared lock); h_counts: host [nq] — what the two synchronous
// searches share: the pre-search verdict, the scratch, index_search with the host reading its words, the flags and the overflow
// word mapped to fallbacks, the statistics.  They differ in
//   lists(&li, &answered)   the lists to walk, fetched only once the pre-search verdict lets the batch search; it may answer the
//                           batch itself (answered: the outputs written, the stream synchronised)
//   pass()                  the exact pass that answers a stale, non-finite, dense or overflowing batch
template <class Lists, class Pass>
int index_sync_search(pg_ctx* ctx, pg_index* ix, bool l2, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc,
                      uint32_t* h_counts, Lists&& lists, Pass&& pass) {
    const pg_table* t = ix->t;
    const uint32_t dim = t->dim;
    IndexPlanWords w{};                  // the plan words as the host read them last (the pairs of the stages scored)
    // the fallback the batch takes
    uint64_t pg_index_stats_t::*fb =
        index_pre_fallback(index_pre_search(t->generation.load(std::memory_order_relaxed), ix->gen, ix->nonfinite, l2, dim));
    int rc = PG_OK;
    if (!fb) rc = [&]() -> int {
        SearchLists li;
        bool answered = false;
        int rc2;
        if ((rc2 = lists(&li, &answered)) || answered) return rc2;
        RecallScratch rs;
        SearchBufs sb;
        if ((rc2 = recall_scratch(ctx, dim, k, &rs))) return rc2;
        if (l2 && (rc2 = ensure_table_nx(ctx, t))) return rc2;
        if (search_bufs(ctx, nq, ix->n_lists, &sb)) {
            fb = &pg_index_stats_t::fallback_overflow;
            return PG_OK;
        }
        if ((rc2 = index_search(ctx, ix, li, d_q, nq, k, l2, rs, sb, d_rows, d_sc, sb.dcount, ~0u, &w))) return rc2;
        if (w.flags & kPlanNonfinite) fb = &pg_index_stats_t::fallback_nonfinite;
        else if (w.flags & kPlanDense) fb = &pg_index_stats_t::fallback_dense;
        if (fb) return PG_OK;
        uint32_t h_ovf = 0;
        PG_HIP(hipMemcpyAsync(&h_ovf, rs.overflow, 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipMemcpyAsync(h_counts, sb.dcount, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        if (h_ovf) fb = &pg_index_stats_t::fallback_overflow;
        return PG_OK;
    }();
    if (rc == PG_OK && fb) rc = pass();
    if (rc != PG_OK) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->st.calls++;
    ix->st.queries += nq;
    ix->st.pairs_scored += w.pairs[0] + w.pairs[1];
    ix->st.rows_scored += w.pairs[0] + w.pairs[1];
    ix->st.rows_live += w.union_rows;
    ix->st.max_query_scan_rows = std::max<uint64_t>(ix->st.max_query_scan_rows, w.max_scan);
    if (fb) ix->st.*fb += 1;
    return PG_OK;
}

// the index's own lists; a fallback is answered by the table's pass
int index_recall_locked(pg_ctx* ctx, pg_index* ix, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc,
                        uint32_t* h_counts, bool l2) {
    return index_sync_search(
        ctx, ix, l2, d_q, nq, k, d_rows, d_sc, h_counts,
        [&](SearchLists* li, bool*) {
            *li = own_lists(ix);
            return PG_OK;
        },
        [&]() { return table_pass_locked(ctx, ix->t, d_q, nq, k, d_rows, d_sc, h_counts, l2); });
}

// pg_index_recall_topk[_l2][_dev]: host, the queries and outputs are host memory (staged through kSlotStaging)
int index_entry(const char* who, pg_ctx* ctx, const pg_index* ixc, const float* q, uint32_t nq, uint32_t k, uint64_t* rows, float* sc,
                uint32_t* out_count, bool l2, bool host) {
    int rc;
    if ((rc = recall_check(who, ctx, ixc, q, rows, sc, nq, k, l2))) return rc;
    pg_index* ix = const_cast<pg_index*>(ixc);          // (only the statistics change)
    std::lock_guard<std::mutex> g(ctx->mu);
    TableRead tr(ix->t->rw);
    uint32_t counts[kMaxQueries];
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return index_recall_locked(ctx, ix, d_q, nq, k, d_rows, d_sc, counts, l2);
    };
    if ((rc = host ? recall_staged(ctx, ix->dim, q, nq, k, rows, sc, run) : run(q, rows, sc))) return rc;
    if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
    return PG_OK;
}

}  // namespace

const pg_table* index_table(const pg_index* ix) { return ix->t; }

pg_index* index_route_where(const pg_ctx* ctx, const pg_table* t) {
    if (!ctx->knobs.index_route_where || t->d_row_map) return nullptr;
    pg_index* ix = t->index.load(std::memory_order_acquire);
    return ix && t->generation.load(std::memory_order_relaxed) == ix->gen ? ix : nullptr;
}

// one filtered batch, synchronously (caller holds ctx->mu and the table's shared lock); h_counts: host [nq].  The search of
// index_recall_locked over the filter's lists; a stale, non-finite, dense or overflowing batch is answered by the filtered pass.
int index_where_locked(pg_ctx* ctx, pg_index* ix, const WhereId& id, const RowFilter& f, bool l2, const float* d_q,
                       uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc, uint32_t* h_counts) {
    std::shared_ptr<WhereLists> wl;      // (released after the stream has synchronised: every path below ends synchronised)
    const int rc = index_sync_search(
        ctx, ix, l2, d_q, nq, k, d_rows, d_sc, h_counts,
        [&](SearchLists* li, bool* answered) -> int {
            int rc2;
            if ((rc2 = where_lists_get(ctx, ix, id, f, &wl))) return rc2;
            if (wl->admitted == 0) {
                // nothing passes: padding, every count 0 (as pg_recall_topk_where)
                if ((rc2 = where_pad_launch(ctx, d_rows, d_sc, (size_t)nq * k, l2))) return rc2;
                for (uint32_t q = 0; q < nq; ++q) h_counts[q] = 0;
                PG_HIP(hipStreamSynchronize(ctx->stream));
                *answered = true;
                return PG_OK;
            }
            // the dense rule weighs the pairs against the filtered pass, which streams the table or gathers a compact copy of the
            // admitted rows, whichever is less
            *li = SearchLists{wl->perm, wl->off, wl->admitted, std::min((double)ix->rows, kWhereGatherWeight * (double)wl->admitted)};
            return PG_OK;
        },
        [&]() {
            wl.reset();                  // (the search has ended synchronised: the lists go before the filtered pass allocates)
            return recall_where_locked(ctx, ix->t, f, l2 ? 1 : 0, d_q, nq, k, d_rows, d_sc, h_counts);
        });
    if (rc != PG_OK && wl) (void)hipStreamSynchronize(ctx->stream);      // (a search that failed under way: before wl goes)
    return rc;
}

// ---- an attached index as a RecallJob plan ------------------------------------------------------------------------
// In front of the table's plans when the table has an attachment that is current and finite, and the job is one the index
// serves (no filter, not exact_only, not a view, not the index's own fallback or the shard group); the batch's size band may
// be switched off for a while (index_plan_check).  Caller holds ctx->mu and the table's shared lock.
int index_plan_prepare(RecallJob* j) {
    const pg_table* t = j->t;
    j->ix = nullptr;
    j->ix_serve.reset();
    pg_index* ix = t->index.load(std::memory_order_acquire);
    if (!ix || j->no_index || j->filter.col || j->exact_only || j->skip_pilot || t->d_row_map) return PG_OK;
    IndexServe& sv = *ix->serve;
    const IndexPre pre = index_pre_search(t->generation.load(std::memory_order_relaxed), ix->gen, ix->nonfinite, j->l2, t->dim);
    if (pre == IndexPre::stale) sv.skipped_stale++;
    if (pre != IndexPre::search || j->k > 16384 || (!j->l2 && t->dim > 128 && j->nq > 32)) return PG_OK;
    if (serve_take_skip(sv, j->nq)) return PG_OK;
    SearchBufs room;
    if (search_bufs(j->ctx, j->nq, ix->n_lists, &room)) return PG_OK;     // (no memory: the table's plans)
    for (int i = j->n_plans; i > 0; --i) j->plans[i] = j->plans[i - 1];
    j->plans[0] = kIndexPlan;
    j->n_plans++;
    j->next_plan = 0;
    j->ix = ix;
    j->ix_serve = ix->serve;
    return PG_OK;
}

// index_search with the attached plan's round policy (index_plan_rounds per stage, no host reads) between the job's events; the
// outputs, the status block and its copy as any plan's
int index_plan_enqueue(RecallJob* j, uint32_t status_words) {
    pg_ctx* ctx = j->ctx;
    const uint32_t nq = j->nq;
    RecallScratch& rs = j->rs;
    hipStream_t s = ctx->stream;
    int rc;
    SearchBufs sb;
    if ((rc = search_bufs(ctx, nq, j->ix->n_lists, &sb))) return rc;      // (reserved by index_plan_prepare: only grows)
    while (j->events->size() < 2) {
        hipEvent_t e;
        PG_HIP(hipEventCreate(&e));
        j->events->push_back(e);
    }
    j->timers = !ctx->timers_off;
    if (j->timers) PG_HIP(hipEventRecord((*j->events)[0], s));
    const uint32_t budget = ctx->knobs.index_plan_rounds ? ctx->knobs.index_plan_rounds : 1u;
    if ((rc = index_search(ctx, j->ix, own_lists(j->ix), j->d_queries, nq, j->k, j->l2, rs, sb, j->d_out_rows, j->d_out_scores, j->d_count, budget, nullptr)))
        return rc;
    if (j->timers) PG_HIP(hipEventRecord((*j->events)[1], s));
    index_status_kernel<<<1, kMaxQueries, 0, s>>>(rs.overflow, nq, sb.pw, rs.status);
    PG_HIP(hipGetLastError());
    if (j->d_out_count) PG_HIP(hipMemcpyAsync(j->d_out_count, j->d_count, 4 * (size_t)nq, hipMemcpyDeviceToDevice, s));
    PG_HIP(hipMemcpyAsync(j->h_status, rs.status, 4 * (size_t)status_words, hipMemcpyDeviceToHost, s));
    j->n_ev = 1;
    j->refined = j->observed = j->susp_stat = j->stat_wide = false;
    j->enqueued_plan = kIndexPlan;
    j->next_plan++;
    return PG_OK;
}

// the verdict of an enqueued index plan (its status words have arrived): held, or a reason to let the table's first plan serve
// the whole batch — dense and rounds also switch the batch's size band off for index_skip_batches batches
int index_plan_check(RecallJob* j, bool* ok) {
    IndexServe& sv = *j->ix_serve;
    IndexPlanWords w;
    memcpy(&w, j->h_status + kIndexStatAt, sizeof w);
    j->failed.clear();
    *ok = serve_plan_done(sv, j->nq, w.flags, j->h_status[0], j->ctx->knobs.index_skip_batches, w.pairs[0] + w.pairs[1], w.union_rows,
                          w.max_scan) == PlanVerdict::held;
    if (j->ctx->knobs.debug_scan)
        fprintf(stderr, "[pg] index plan %s: flags %u, rounds %u + %u, pairs %llu + %llu\n", *ok ? "held" : "re-planned", w.flags, w.need[0],
                w.need[1], w.pairs[0], w.pairs[1]);
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_index_recall_topk(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                         float* out_scores, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk", ctx, ix, queries, nq, k, out_rows, out_scores, out_count, false, true);
}

int pg_index_recall_topk_dev(pg_ctx* ctx, const pg_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                             float* d_out_scores, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk_dev", ctx, ix, d_queries, nq, k, d_out_rows, d_out_scores, out_count, false, false);
}

int pg_index_recall_topk_l2(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                            float* out_dist, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk_l2", ctx, ix, queries, nq, k, out_rows, out_dist, out_count, true, true);
}

int pg_index_recall_topk_l2_dev(pg_ctx* ctx, const pg_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                                float* d_out_dist, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk_l2_dev", ctx, ix, d_queries, nq, k, d_out_rows, d_out_dist, out_count, true, false);
}

// the filtered recall through the index: pg_recall_topk_where's checks and contract, over ix's table
int pg_index_recall_topk_where(pg_ctx* ctx, const pg_index* ixc, const pg_features* fs, int column, int op, long long value, int metric,
                               const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(ixc, "pg_index_recall_topk_where: NULL argument");
    pg::RowFilter f;
    int rc;
    if ((rc = pg::where_check("pg_index_recall_topk_where", ctx, ixc->t, fs, column, op, value, metric, queries, out_rows, out_scores, nq, k,
                              &f)))
        return rc;
    pg_index* ix = const_cast<pg_index*>(ixc);          // (only the statistics and the filtered lists' cache change)
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);
    uint32_t counts[pg::kMaxQueries];
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return pg::index_where_locked(ctx, ix, pg::WhereId{fs, column, nullptr, 0}, f, metric == 1, d_q, nq, k, d_rows, d_sc, counts);
    };
    if ((rc = pg::recall_staged(ctx, ix->dim, queries, nq, k, out_rows, out_scores, run))) return rc;
    if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
    return PG_OK;
}

int pg_index_stats(const pg_index* ixc, pg_index_stats_t* out) {
    PG_REQUIRE(ixc && out, "pg_index_stats: NULL argument");
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ix->mu);
    *out = ix->st;
    pg::serve_fold_stats(*ix->serve, out);       // (+ the batches that tried the attached plan)
    return PG_OK;
}

// Attach / detach change no rows: the table's lock is taken exclusively WITHOUT a generation bump (TableWrite's), and the
// device is drained so that nothing enqueued still reads a previous attachment's arrays.
int pg_index_attach(pg_ctx* ctx, pg_index* ix) {
    PG_REQUIRE(ctx && ix, "pg_index_attach: NULL argument");
    PG_REQUIRE(!ix->t->d_row_map, "pg_index_attach: the table is a view");
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> w(ix->t->rw);
    pg_index* prev = ix->t->index.load(std::memory_order_acquire);
    if (prev == ix) return PG_OK;
    if (prev) {
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipDeviceSynchronize());
    }
    ix->t->index.store(ix, std::memory_order_release);
    return PG_OK;
}

int pg_index_detach(pg_ctx* ctx, pg_index* ix) {
    PG_REQUIRE(ctx && ix, "pg_index_detach: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> w(ix->t->rw);
    PG_REQUIRE(ix->t->index.load(std::memory_order_acquire) == ix, "pg_index_detach: the index is not attached");
    PG_HIP(hipSetDevice(ctx->device));
    PG_HIP(hipDeviceSynchronize());
    ix->t->index.store(nullptr, std::memory_order_release);
    return PG_OK;
}

int pg_index_serving_stats(const pg_index* ix, pg_index_serving_stats_t* out) {
    PG_REQUIRE(ix && out, "pg_index_serving_stats: NULL argument");
    const pg::IndexServe& sv = *ix->serve;
    out->plans = sv.plans.load();
    out->plans_held = sv.plans_held.load();
    out->queries_held = sv.queries_held.load();
    out->replan_dense = sv.replan_dense.load();
    out->replan_rounds = sv.replan_rounds.load();
    out->replan_overflow = sv.replan_overflow.load();
    out->replan_nonfinite = sv.replan_nonfinite.load();
    out->skipped_stale = sv.skipped_stale.load();
    out->skipped_switch = sv.skipped_switch.load();
    return PG_OK;
}

}  // extern "C"
