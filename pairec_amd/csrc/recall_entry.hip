// recall_entry.hip — the recalls as their callers see them: one verified batch of queries (recall_dev_locked: the plans of
// recall_plan.hip, enqueued, synchronised and checked), batches of batches, host staging, per-request exclusion lists, and the pg_*
// entry points of VectorRecall (service/recall/vector_recall.go:88-102), HologresVectorRecallV2
// (hologres_vector_recall_v2.go:23,96-206), I2IVectorRecall (item_2_item_vector_racall.go:51-152) and OnlineVectorRecall
// (online_vector_recall.go:73-155).  Host code only: every kernel is behind a function of common.hpp.
#include "common.hpp"

namespace pg {

// the whole recall for one batch of queries, verified before it returns; all pointers are device pointers
int recall_dev_locked(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq,
                      uint32_t k, uint64_t* d_out_rows, float* d_out_scores,
                      uint32_t* out_count, uint32_t* d_out_count, const RecallOpts& o) {
    RecallJob j;
    j.exact_only = o.exact_only;
    j.no_index = o.no_index;
    j.skip_pilot = o.skip_pilot;
    j.l2 = o.l2;
    if (o.filter) j.filter = *o.filter;
    j.ctx = ctx;
    j.t = t;
    j.d_queries = d_queries;
    j.nq = nq;
    j.k = k;
    j.d_out_rows = d_out_rows;
    j.d_out_scores = d_out_scores;
    j.d_out_count = d_out_count;
    j.h_status = ctx->h_status;
    j.events = &ctx->ev_pool;
    int rc;
    if ((rc = recall_job_prepare(&j))) return rc;
    uint32_t counts[kMaxQueries];
    for (;;) {
        if ((rc = recall_job_enqueue(&j))) return rc;
        PG_HIP(hipStreamSynchronize(ctx->stream));
        bool ok = false;
        if ((rc = recall_job_check(&j, &ok))) return rc;
        for (uint32_t q = 0; q < nq; ++q) counts[q] = ctx->h_status[1 + q];
        if (ok) break;
        if (!j.failed.empty() && j.failed.size() <= kMaxPatchQueries && nq > 1) {
            // the pilot's threshold was too high for a few queries only: re-run those, not the batch
            // (the nested calls reuse ctx->h_status: the counts are kept on the stack)
            if ((rc = recall_patch_failed_locked(&j, counts))) return rc;
            break;
        }
    }
    if (out_count)
        for (uint32_t q = 0; q < nq; ++q) out_count[q] = counts[q];
    recall_job_finish(&j);
    return PG_OK;
}

int recall_batches_locked(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                          float* d_out_scores, uint32_t* out_count, const RecallOpts& o) {
    const uint32_t step = o.l2 ? 128u : (uint32_t)kMaxQueries;
    for (uint32_t q0 = 0; q0 < nq; q0 += step) {
        const uint32_t n = nq - q0 < step ? nq - q0 : step;
        const int rc = recall_dev_locked(ctx, t, d_queries + (size_t)q0 * t->dim, n, k, d_out_rows + (size_t)q0 * k,
                                         d_out_scores + (size_t)q0 * k, out_count ? out_count + q0 : nullptr, nullptr, o);
        if (rc) return rc;
    }
    return PG_OK;
}

// pg_recall_topk[_l2][_dev]: host, the queries and outputs are host memory (staged through kSlotStaging)
int recall_entry(const char* who, pg_ctx* ctx, const pg_table* t, const float* q, uint32_t nq, uint32_t k, uint64_t* rows, float* sc,
                 uint32_t* out_count, bool l2, bool host) {
    int rc;
    if ((rc = recall_check(who, ctx, t, q, rows, sc, nq, k, l2))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    TableRead tr(t->rw);
    RecallOpts o;
    o.l2 = l2;
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return recall_batches_locked(ctx, t, d_q, nq, k, d_rows, d_sc, out_count, o);
    };
    return host ? recall_staged(ctx, t->dim, q, nq, k, rows, sc, run) : run(q, rows, sc);
}

// ---- recalls with per-request exclusion lists (the kernel: exclude.hip) ----------------------------------------
// The offsets of nq lists (`extra` more ids join every list: the request's own trigger row): monotone, at most kMaxExclude ids
// each, k + the longest within the recalls' 16384.
int exclude_lists_check(const char* who, const uint32_t* off, uint32_t nq, uint32_t k, uint32_t extra, uint32_t* nmax_out) {
    uint32_t nmax = extra;
    for (uint32_t q = 0; off && q < nq; ++q) {
        PG_REQUIRE(off[q + 1] >= off[q], "%s: excl_offsets[%u] = %u is below excl_offsets[%u] = %u", who, q + 1, off[q + 1], q, off[q]);
        if (off[q + 1] - off[q] > kMaxExclude) {
            set_error("%s: request %u excludes %u ids (at most %u per request)", who, q, off[q + 1] - off[q], kMaxExclude);
            return PG_ERR_UNSUPPORTED;
        }
        nmax = std::max(nmax, off[q + 1] - off[q] + extra);
    }
    if (nmax > kMaxExclude) {
        set_error("%s: a list of %u ids with the trigger row (at most %u per request)", who, nmax, kMaxExclude);
        return PG_ERR_UNSUPPORTED;
    }
    if ((uint64_t)k + nmax > 16384) {
        set_error("%s: k=%u plus the longest exclusion list of %u ids exceeds the recalls' depth of 16384", who, k, nmax);
        return PG_ERR_UNSUPPORTED;
    }
    *nmax_out = nmax;
    return PG_OK;
}

// One recall of nq device queries at depth k + nmax through `inner` — the plain call's own search — into kSlotRecallExclude, then
// the compaction into d_rows / d_sc [nq][k].  excl: the lists' ids, host (staged here, off rebased) or device (indexed by off
// as given); off: host [nq + 1].  nmax = 0: `inner` at k straight into the outputs.  Caller holds ctx->mu and the table's
// shared lock; ends synchronised (out_count: host [nq] or NULL).
template <class Inner>
int recall_exclude_locked(pg_ctx* ctx, uint32_t nq, uint32_t k, uint32_t nmax, bool l2, const uint64_t* excl, bool excl_on_host,
                          const uint32_t* off, uint64_t* d_rows, float* d_sc, uint32_t* out_count, Inner&& inner) {
    int rc;
    uint32_t counts[kMaxQueries];
    if (nmax == 0) {
        if ((rc = inner(k, d_rows, d_sc, counts))) return rc;
        if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
        return PG_OK;
    }
    const uint32_t kx = k + nmax;
    const uint32_t total = excl_on_host ? off[nq] - off[0] : 0;
    uint32_t *d_off, *d_cnt; uint64_t *d_list, *d_xrows; float* d_xsc;
    if ((rc = scratch_carve(ctx, kSlotRecallExclude, [&](Carve& c) {
            d_off = c.take<uint32_t>((size_t)nq + 1);
            d_cnt = c.take<uint32_t>(nq);
            d_list = c.take<uint64_t>(total);
            d_xrows = c.take<uint64_t>((size_t)nq * kx);
            d_xsc = c.take<float>((size_t)nq * kx);
        }))) return rc;
    uint32_t h_off[kMaxQueries + 1];
    for (uint32_t q = 0; q <= nq; ++q) h_off[q] = excl_on_host ? off[q] - off[0] : off[q];
    PG_HIP(hipMemcpyAsync(d_off, h_off, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (total) PG_HIP(hipMemcpyAsync(d_list, excl + off[0], (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));          // (h_off lives on this frame, and the inner recall may reuse pageable staging)
    if ((rc = inner(kx, d_xrows, d_xsc, counts))) return rc;
    if ((rc = exclude_compact_locked(ctx, d_xrows, d_xsc, nq, kx, excl_on_host ? d_list : excl, d_off, k,
                                     l2 ? __builtin_inff() : -__builtin_inff(), d_rows, d_sc, d_cnt)))
        return rc;
    PG_HIP(hipMemcpyAsync(ctx->h_status, d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    if (out_count) memcpy(out_count, ctx->h_status, (size_t)nq * 4);
    return PG_OK;
}

// the queries of an item-to-item recall arrive as rows of the trigger table: the trigger rows are few, one small
// device-to-device copy each (coalesced 512-B rows)
int trigger_fill(pg_ctx* ctx, const pg_table* trigger_table, const uint32_t* trigger_rows, uint32_t n, float* d_q) {
    const size_t dim = trigger_table->dim;
    for (uint32_t i = 0; i < n; ++i)
        PG_HIP(hipMemcpyAsync(d_q + i * dim, trigger_table->d + trigger_rows[i] * dim, dim * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return PG_OK;
}

// pg_recall_topk_exclude[_dev]: the checks of the call it extends (pg_recall_topk[_l2][_dev], or pg_recall_topk_where_ex with a
// clause), then the lists'
int recall_exclude_entry(const char* who, pg_ctx* ctx, const pg_table* t, const float* q, uint32_t nq, uint32_t k, const uint64_t* excl,
                         const uint32_t* off, const pg_recall_exclude_opts* opts, uint64_t* rows, float* sc, uint32_t* out_count, bool host) {
    const int metric = opts ? opts->metric : 0;
    const pg_features* fs = opts ? opts->fs : nullptr;
    const pg_where* w = opts ? opts->where : nullptr;
    PG_REQUIRE((fs != nullptr) == (w != nullptr), "%s: opts->fs and opts->where come together", who);
    int rc;
    if (w) {
        if ((rc = where_clause_check(who, ctx, t, fs, w, metric, q, rows, sc, nq, k))) return rc;
    } else {
        PG_REQUIRE(metric == 0 || metric == 1, "%s: metric %d unknown (0 inner product, 1 squared Euclidean)", who, metric);
        if ((rc = recall_check(who, ctx, t, q, rows, sc, nq, k, metric == 1))) return rc;
    }
    PG_REQUIRE(off, "%s: excl_offsets is NULL", who);
    uint32_t nmax = 0;
    if ((rc = exclude_lists_check(who, off, nq, k, 0, &nmax))) return rc;
    PG_REQUIRE(excl || off[nq] == off[0], "%s: excl_rows is NULL", who);
    std::lock_guard<std::mutex> g(ctx->mu);
    TableRead tr(t->rw);
    WhereServe ws;
    if (w && (rc = where_clause_bind(who, ctx, t, fs, w, &ws))) return rc;
    pg_index* ix = w ? index_route_where(ctx, t) : nullptr;
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        auto inner = [&](uint32_t kk, uint64_t* r, float* s, uint32_t* counts) {
            if (!w) {
                RecallOpts o;
                o.l2 = metric == 1;
                return recall_batches_locked(ctx, t, d_q, nq, kk, r, s, counts, o);
            }
            return ix ? index_where_locked(ctx, ix, ws.id, ws.f, metric == 1, d_q, nq, kk, r, s, counts)
                      : recall_where_locked(ctx, t, ws.f, metric, d_q, nq, kk, r, s, counts);
        };
        return recall_exclude_locked(ctx, nq, k, nmax, metric == 1, excl, host, off, d_rows, d_sc, out_count, inner);
    };
    rc = host ? recall_staged(ctx, t->dim, q, nq, k, rows, sc, run) : run(q, rows, sc);
    if (rc != PG_OK && w) (void)hipStreamSynchronize(ctx->stream);      // (nothing enqueued reads the bitmap once ws lets go of it)
    return rc;
}

}  // namespace pg

extern "C" {

int pg_recall_topk_dev(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq,
                       uint32_t k, uint64_t* d_out_rows, float* d_out_scores, uint32_t* out_count) {
    return pg::recall_entry("pg_recall_topk_dev", ctx, t, d_queries, nq, k, d_out_rows, d_out_scores, out_count, false, false);
}

int pg_recall_topk(pg_ctx* ctx, const pg_table* t, const float* queries, uint32_t nq, uint32_t k,
                   uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    return pg::recall_entry("pg_recall_topk", ctx, t, queries, nq, k, out_rows, out_scores, out_count, false, true);
}

// HologresVectorRecallV2 (service/recall/hologres_vector_recall_v2.go:23,96-206): "SELECT id, pm_approx_squared_euclidean_distance
// (emb, $1) as distance … ORDER BY distance LIMIT n" — the K rows of SMALLEST squared Euclidean distance, ascending, the distance
// as the item's score (:181-189).  Exact here (the reference's Proxima index is approximate): d = fmaf(-2, ip, |x|^2 + |q|^2),
// every sum a k-ascending fp32 fmaf chain; ties by row ascending; slots beyond the table's rows: row UINT64_MAX, distance +inf.
int pg_recall_topk_l2_dev(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                          float* d_out_dist, uint32_t* out_count) {
    return pg::recall_entry("pg_recall_topk_l2_dev", ctx, t, d_queries, nq, k, d_out_rows, d_out_dist, out_count, true, false);
}

int pg_recall_topk_l2(pg_ctx* ctx, const pg_table* t, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                      float* out_dist, uint32_t* out_count) {
    return pg::recall_entry("pg_recall_topk_l2", ctx, t, queries, nq, k, out_rows, out_dist, out_count, true, true);
}

// I2IVectorRecall (service/recall/item_2_item_vector_racall.go:51-152): the trigger item's own embedding
// (dao.VectorString(item_id)) is the query of the same inner-product top-K; the trigger is not excluded (the
// reference's SQL does not exclude it either).
int pg_i2i_recall(pg_ctx* ctx, const pg_table* trigger_table, const uint32_t* trigger_rows, uint32_t n,
                  const pg_table* t, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(ctx && trigger_table && t && trigger_rows && out_rows && out_scores, "pg_i2i_recall: NULL argument");
    PG_REQUIRE(trigger_table->dim == t->dim, "pg_i2i_recall: trigger table dim %u != searched table dim %u", trigger_table->dim, t->dim);
    PG_REQUIRE(!trigger_table->d_row_map, "pg_i2i_recall: the trigger table is a filtered view (trigger rows are rows of the source)");
    PG_REQUIRE(n >= 1 && n <= (uint32_t)pg::kMaxQueries && (t->dim <= 128 || n <= 32), "pg_i2i_recall: %u trigger items per call unsupported", n);
    if (k < 1 || k > 16384) {
        pg::set_error("pg_i2i_recall: k=%u unsupported (1..16384)", k);
        return PG_ERR_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < n; ++i)
        PG_REQUIRE(trigger_rows[i] < trigger_table->rows, "pg_i2i_recall: trigger row %u outside table of %llu rows", trigger_rows[i],
                   (unsigned long long)trigger_table->rows);
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead2 tr(t, trigger_table);
    auto fill = [&](float* d_q) { return pg::trigger_fill(ctx, trigger_table, trigger_rows, n, d_q); };
    return pg::recall_staged(ctx, t->dim, nullptr, n, k, out_rows, out_scores, [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return pg::recall_dev_locked(ctx, t, d_q, n, k, d_rows, d_sc, out_count, nullptr);
    }, fill);
}

int pg_recall_topk_exclude(pg_ctx* ctx, const pg_table* t, const float* queries, uint32_t nq, uint32_t k, const uint64_t* excl_rows,
                           const uint32_t* excl_offsets, const pg_recall_exclude_opts* opts, uint64_t* out_rows, float* out_scores,
                           uint32_t* out_count) {
    return pg::recall_exclude_entry("pg_recall_topk_exclude", ctx, t, queries, nq, k, excl_rows, excl_offsets, opts, out_rows, out_scores,
                                    out_count, true);
}

int pg_recall_topk_exclude_dev(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k, const uint64_t* d_excl_rows,
                               const uint32_t* excl_offsets, const pg_recall_exclude_opts* opts, uint64_t* d_out_rows, float* d_out_scores,
                               uint32_t* out_count) {
    return pg::recall_exclude_entry("pg_recall_topk_exclude_dev", ctx, t, d_queries, nq, k, d_excl_rows, excl_offsets, opts, d_out_rows,
                                    d_out_scores, out_count, false);
}

// pg_i2i_recall without the items the request has seen — and, with exclude_trigger, without the trigger item itself (the hole
// pg_i2i_recall documents): its checks in its order, then the lists'
int pg_i2i_recall_exclude(pg_ctx* ctx, const pg_table* trigger_table, const uint32_t* trigger_rows, uint32_t n, const pg_table* t,
                          uint32_t k, int exclude_trigger, const uint64_t* excl_rows, const uint32_t* excl_offsets, uint64_t* out_rows,
                          float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(ctx && trigger_table && t && trigger_rows && out_rows && out_scores, "pg_i2i_recall_exclude: NULL argument");
    PG_REQUIRE(trigger_table->dim == t->dim, "pg_i2i_recall_exclude: trigger table dim %u != searched table dim %u", trigger_table->dim, t->dim);
    PG_REQUIRE(!trigger_table->d_row_map, "pg_i2i_recall_exclude: the trigger table is a filtered view (trigger rows are rows of the source)");
    PG_REQUIRE(n >= 1 && n <= (uint32_t)pg::kMaxQueries && (t->dim <= 128 || n <= 32), "pg_i2i_recall_exclude: %u trigger items per call unsupported", n);
    if (k < 1 || k > 16384) {
        pg::set_error("pg_i2i_recall_exclude: k=%u unsupported (1..16384)", k);
        return PG_ERR_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < n; ++i)
        PG_REQUIRE(trigger_rows[i] < trigger_table->rows, "pg_i2i_recall_exclude: trigger row %u outside table of %llu rows", trigger_rows[i],
                   (unsigned long long)trigger_table->rows);
    PG_REQUIRE(!exclude_trigger || trigger_table == t, "pg_i2i_recall_exclude: exclude_trigger needs the trigger table to be the searched table");
    PG_REQUIRE(excl_offsets || exclude_trigger, "pg_i2i_recall_exclude: excl_offsets is NULL");
    uint32_t nmax = 0;
    int rc;
    if ((rc = pg::exclude_lists_check("pg_i2i_recall_exclude", excl_offsets, n, k, exclude_trigger ? 1u : 0u, &nmax))) return rc;
    PG_REQUIRE(excl_rows || !excl_offsets || excl_offsets[n] == excl_offsets[0], "pg_i2i_recall_exclude: excl_rows is NULL");
    // every request's list with its trigger row behind it
    std::vector<uint64_t> lists;
    std::vector<uint32_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (excl_offsets) lists.insert(lists.end(), excl_rows + excl_offsets[i], excl_rows + excl_offsets[i + 1]);
        if (exclude_trigger) lists.push_back(t->row_offset + trigger_rows[i]);
        off[i + 1] = (uint32_t)lists.size();
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead2 tr(t, trigger_table);
    auto fill = [&](float* d_q) { return pg::trigger_fill(ctx, trigger_table, trigger_rows, n, d_q); };
    return pg::recall_staged(ctx, t->dim, nullptr, n, k, out_rows, out_scores, [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        auto inner = [&](uint32_t kk, uint64_t* r, float* s, uint32_t* counts) { return pg::recall_dev_locked(ctx, t, d_q, n, kk, r, s, counts, nullptr); };
        return pg::recall_exclude_locked(ctx, n, k, nmax, false, lists.data(), true, off.data(), d_rows, d_sc, out_count, inner);
    }, fill);
}

// OnlineVectorRecall (service/recall/online_vector_recall.go:73-155): the model server turns the user's features
// into the user-tower embedding and answers with its FaissNeighNum nearest items (match_item_scores + item_ids,
// algorithm/eas/easyrec_response.go:700-734).  Here: user tower of the two-tower model on the device, then the
// same exact inner-product top-K over the item-embedding table (dim = the towers' output width).
int pg_online_vector_recall(pg_ctx* ctx, const pg_model* m, const pg_table* item_emb, const float* user_vecs,
                            uint32_t n_req, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(ctx && m && item_emb && user_vecs && out_rows && out_scores, "pg_online_vector_recall: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_online_vector_recall: model is not FM_TWOTOWER");
    PG_REQUIRE(item_emb->dim == m->to, "pg_online_vector_recall: item-embedding table dim %u != tower output %u", item_emb->dim, m->to);
    PG_REQUIRE(n_req >= 1 && n_req <= (uint32_t)pg::kMaxQueries, "pg_online_vector_recall: n_req=%u must be in [1,%d]", n_req, pg::kMaxQueries);
    if (k < 1 || k > 16384) {
        pg::set_error("pg_online_vector_recall: k=%u unsupported (1..16384)", k);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(item_emb->rw);
    float *d_u, *d_q, *d_sc;
    uint64_t* d_rows;
    int rc;
    const size_t rb = (size_t)n_req * k * 8, sb = (size_t)n_req * k * 4;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& c) {
            d_u = c.take<float>((size_t)n_req * m->d_user);
            d_q = c.take<float>((size_t)n_req * m->to);
            d_rows = c.take<uint64_t>((size_t)n_req * k);
            d_sc = c.take<float>((size_t)n_req * k);
        }))) return rc;
    PG_HIP(hipMemcpyAsync(d_u, user_vecs, (size_t)n_req * m->d_user * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pg::fm2t_user_embedding_locked(ctx, m, d_u, n_req, d_q))) return rc;
    if ((rc = pg::recall_dev_locked(ctx, item_emb, d_q, n_req, k, d_rows, d_sc, out_count, nullptr))) return rc;
    PG_HIP(hipMemcpyAsync(out_rows, d_rows, rb, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(out_scores, d_sc, sb, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

}  // extern "C"
