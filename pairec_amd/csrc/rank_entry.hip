// rank_entry.hip — the rank stage's entry points: pg_model_load (rank_model.hpp reads the blob and lists what goes to the
// device), the host-buffer rank calls and their *_dev forms, the item records' life cycle.  Nothing here launches a kernel:
// the launches are rank_mlp.hip's *_locked functions (common.hpp).
#include "rank_mlp.hpp"

#include <memory>

namespace pg {

static int upload(pg_ctx* ctx, pg_model* m, const void* src, size_t bytes, void** dst) {
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes ? bytes : 16);
    if (e != hipSuccess) {
        set_error("pg_model_load: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return PG_ERR_NOMEM;
    }
    m->allocs.push_back(d);
    if (bytes) PG_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    *dst = d;
    return PG_OK;
}

static int finish_rank_timing(pg_ctx* ctx) {
    PG_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->rank_timing_pending) return PG_OK;       // (stage timers off: nothing was recorded, last_rank_ms stays)
    float ms = 0.f;
    PG_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
    ctx->stats.last_rank_ms = ms;
    ctx->rank_timing_pending = false;
    return PG_OK;
}

// One input of a host-buffer rank call: `count` elements of `elem` bytes per request (or per candidate), copied from `host` —
// or, with copy false, only carved: the entry fills it on the device.
struct HostIn {
    const void* host;
    bool per_item;
    size_t count, elem;
    bool copy = true;
};
static int no_check(uint32_t) { return PG_OK; }

// What the host-buffer rank entries share, in the name of the entry `who`: the request limit and the offsets' checks, the early
// returns of an empty call, the NULL check of what a non-empty call reads, the user field ids' range (two-tower entries pass
// them), check(n_items) — the entry's own range checks; then, under ctx->mu and with `t` (DNN3) held for reading, the inputs
// staged in kSlotStaging in list order, behind them the offsets and the scores, run(d_in, d_off, n_items, d_scores) with d_in
// the inputs' device addresses in list order, the scores copied out and the rank timer read.
template <size_t N, class Check, class Run>
static int rank_from_host(const char* who, pg_ctx* ctx, const pg_model* m, const pg_table* t, const HostIn (&in)[N],
                          const int32_t* user_field_ids, const uint32_t* req_offsets, uint32_t n_req, float* out_scores,
                          Check&& check, Run&& run) {
    PG_REQUIRE(n_req <= 65535, "%s: at most 65535 requests per call", who);
    if (n_req == 0) return PG_OK;
    PG_REQUIRE(req_offsets[0] == 0, "%s: req_offsets[0] must be 0", who);
    for (uint32_t r = 0; r < n_req; ++r)
        PG_REQUIRE(req_offsets[r + 1] >= req_offsets[r], "%s: req_offsets not monotone at %u", who, r);
    const uint32_t n_items = req_offsets[n_req];
    if (n_items == 0) return PG_OK;
    bool given = out_scores != nullptr;
    for (const HostIn& i : in) given = given && (i.host || !i.copy);
    PG_REQUIRE(given, "%s: NULL argument", who);
    if (user_field_ids)
        for (size_t i = 0; i < (size_t)n_req * m->nuf; ++i)
            PG_REQUIRE(user_field_ids[i] >= 0 && (uint32_t)user_field_ids[i] < m->vocab, "%s: user field id %d outside vocab %u", who,
                       user_field_ids[i], m->vocab);
    int rc;
    if ((rc = check(n_items))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    TableRead tr;
    if (t) tr = TableRead(t->rw);
    void* d_in[N];
    size_t bytes[N];
    uint32_t* d_o;
    float* d_s;
    const size_t ob = (size_t)(n_req + 1) * 4, sb = (size_t)n_items * 4 * m->n_out;
    for (size_t i = 0; i < N; ++i) bytes[i] = (in[i].per_item ? n_items : n_req) * in[i].count * in[i].elem;
    if ((rc = scratch_carve(ctx, kSlotStaging, [&](Carve& c) {
            for (size_t i = 0; i < N; ++i) d_in[i] = c.bytes(bytes[i]);
            d_o = c.take<uint32_t>(ob / 4);
            d_s = c.take<float>(sb / 4);
        }))) return rc;
    for (size_t i = 0; i < N; ++i)
        if (in[i].copy) PG_HIP(hipMemcpyAsync(d_in[i], in[i].host, bytes[i], hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipMemcpyAsync(d_o, req_offsets, ob, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run(d_in, d_o, n_items, d_s))) return rc;
    PG_HIP(hipMemcpyAsync(out_scores, d_s, sb, hipMemcpyDeviceToHost, ctx->stream));
    return finish_rank_timing(ctx);
}

}  // namespace pg

extern "C" {

int pg_model_load(pg_ctx* ctx, pg_model_kind kind, pg_prec prec, const void* blob, size_t len,
                  pg_model** out) {
    PG_REQUIRE(ctx && blob && out, "pg_model_load: NULL argument");
    auto m = std::make_unique<pg_model>();
    m->ctx = ctx;
    pg::BlobLayout lay;
    pg::ModelUploads up;
    pg::ModelRefusal why;
    if (pg::parse_model_blob(kind, prec, blob, len, m.get(), &lay, &why) || pg::model_uploads(m.get(), lay, blob, &up, &why)) {
        pg::set_error("%s", why.text);
        return why.status;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    int rc;
    auto fail = [&](int code) {
        for (void* a : m->allocs) hipFree(a);
        return code;
    };
    for (const pg::ModelUpload& u : up.list) {
        void* d;
        if ((rc = pg::upload(ctx, m.get(), u.src, u.bytes, &d))) return fail(rc);
        pg::model_upload_placed(u, d);
    }
    if (m->kind == PG_MODEL_FM_TWOTOWER) {           // the fields' tables by device address, now that `fields` has one
        const size_t nf = m->nuf + m->nif;
        std::vector<const float*> pe(nf), pl(nf);
        for (size_t f = 0; f < nf; ++f) {
            pe[f] = m->fields + f * ((size_t)m->vocab * m->k + m->vocab);
            pl[f] = pe[f] + (size_t)m->vocab * m->k;
        }
        if ((rc = pg::upload(ctx, m.get(), pe.data(), nf * sizeof(float*), (void**)&m->d_field_emb))) return fail(rc);
        if ((rc = pg::upload(ctx, m.get(), pl.data(), nf * sizeof(float*), (void**)&m->d_field_lin))) return fail(rc);
    }
    *out = m.release();
    return PG_OK;
}

int pg_model_num_outputs(const pg_model* m, uint32_t* out) {
    PG_REQUIRE(m && out, "pg_model_num_outputs: NULL argument");
    *out = m->n_out;
    return PG_OK;
}

int pg_model_f16_stats(const pg_model* m, uint64_t out[4]) {
    PG_REQUIRE(m && out, "pg_model_f16_stats: NULL argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!m->f16_nprod) return PG_OK;
    pg_ctx* ctx = m->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    unsigned long long dev[2] = {0, 0};
    PG_HIP(hipMemcpyAsync(dev, m->h_stats, sizeof dev, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    out[0] = m->f16_calls;
    out[1] = dev[0];
    out[2] = dev[1];
    out[3] = m->f16_calls_whole;
    return PG_OK;
}

int pg_model_destroy(pg_ctx* ctx, pg_model* m) {
    PG_REQUIRE(ctx, "pg_model_destroy: ctx is NULL");
    if (!m) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipStreamSynchronize(ctx->stream));
    for (void* a : m->allocs) PG_HIP(hipFree(a));
    delete m;
    return PG_OK;
}

int pg_rank_dnn3_dev(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user_vecs,
                     const uint32_t* d_cand_rows, const uint32_t* d_req_offsets, uint32_t n_req,
                     uint32_t n_items, float* d_out_scores) {
    PG_REQUIRE(ctx && m && t && d_user_vecs && d_cand_rows && d_req_offsets && d_out_scores,
               "pg_rank_dnn3_dev: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_DNN3, "pg_rank_dnn3_dev: model is not DNN3");
    PG_REQUIRE(t->dim == m->d_item, "pg_rank_dnn3_dev: table dim %u != model d_item %u", t->dim, m->d_item);
    PG_REQUIRE(n_req <= 65535, "pg_rank_dnn3_dev: at most 65535 requests per call");
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    return pg::rank_dnn3_dev_locked(ctx, m, t, d_user_vecs, d_cand_rows, d_req_offsets, n_req, n_items,
                                    d_out_scores);
}

int pg_rank_dnn3(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* user_vecs,
                 const uint32_t* cand_rows, const uint32_t* req_offsets, uint32_t n_req,
                 float* out_scores) {
    PG_REQUIRE(ctx && m && t && req_offsets, "pg_rank_dnn3: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_DNN3, "pg_rank_dnn3: model is not DNN3");
    PG_REQUIRE(t->dim == m->d_item, "pg_rank_dnn3: table dim %u != model d_item %u", t->dim, m->d_item);
    const pg::HostIn in[] = {{user_vecs, false, m->d_user, 4}, {cand_rows, true, 1, 4}};
    return pg::rank_from_host(
        "pg_rank_dnn3", ctx, m, t, in, nullptr, req_offsets, n_req, out_scores,
        [&](uint32_t n_items) -> int {
            for (uint32_t i = 0; i < n_items; ++i)
                PG_REQUIRE(cand_rows[i] < t->rows, "pg_rank_dnn3: candidate %u row %u outside table of %llu rows", i,
                           cand_rows[i], (unsigned long long)t->rows);
            return PG_OK;
        },
        [&](void* const* d, const uint32_t* d_off, uint32_t n_items, float* d_scores) {
            return pg::rank_dnn3_dev_locked(ctx, m, t, (const float*)d[0], (const uint32_t*)d[1], d_off, n_req, n_items, d_scores);
        });
}

int pg_fm2t_user_embedding_dev(pg_ctx* ctx, const pg_model* m, const float* d_user_vecs, uint32_t n_req, float* d_out) {
    PG_REQUIRE(ctx && m && (n_req == 0 || (d_user_vecs && d_out)), "pg_fm2t_user_embedding_dev: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_fm2t_user_embedding_dev: model is not FM_TWOTOWER");
    std::lock_guard<std::mutex> g(ctx->mu);
    return pg::fm2t_user_embedding_locked(ctx, m, d_user_vecs, n_req, d_out);
}

int pg_fm2t_user_embedding(pg_ctx* ctx, const pg_model* m, const float* user_vecs, uint32_t n_req, float* out) {
    PG_REQUIRE(ctx && m && (n_req == 0 || (user_vecs && out)), "pg_fm2t_user_embedding: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_fm2t_user_embedding: model is not FM_TWOTOWER");
    if (n_req == 0) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    float *d_u, *d_o;
    int rc;
    const size_t ob = (size_t)n_req * m->to * 4;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& c) {
            d_u = c.take<float>((size_t)n_req * m->d_user);
            d_o = c.take<float>(ob / 4);
        }))) return rc;
    PG_HIP(hipMemcpyAsync(d_u, user_vecs, (size_t)n_req * m->d_user * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pg::fm2t_user_embedding_locked(ctx, m, d_u, n_req, d_o))) return rc;
    PG_HIP(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_rank_fm2t_dev(pg_ctx* ctx, const pg_model* m, const float* d_user_vecs,
                     const int32_t* d_user_field_ids, const int32_t* d_item_field_ids,
                     const uint32_t* d_req_offsets, uint32_t n_req, uint32_t n_items,
                     float* d_out_scores) {
    PG_REQUIRE(ctx && m && d_user_vecs && d_user_field_ids && d_item_field_ids && d_req_offsets && d_out_scores,
               "pg_rank_fm2t_dev: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_rank_fm2t_dev: model is not FM_TWOTOWER");
    PG_REQUIRE(n_req <= 65535, "pg_rank_fm2t_dev: at most 65535 requests per call");
    std::lock_guard<std::mutex> g(ctx->mu);
    return pg::rank_fm2t_dev_locked(ctx, m, d_user_vecs, d_user_field_ids, d_item_field_ids, d_req_offsets,
                                    n_req, n_items, d_out_scores);
}

int pg_rank_fm2t_rows_dev(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                          const float* d_user_vecs, const int32_t* d_user_field_ids, const uint32_t* d_cand_rows,
                          const uint32_t* d_req_offsets, uint32_t n_req, uint32_t n_items, float* d_out_scores) {
    PG_REQUIRE(ctx && m && fs && item_field_cols && d_user_vecs && d_user_field_ids && d_cand_rows && d_req_offsets &&
                   d_out_scores,
               "pg_rank_fm2t_rows_dev: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_rank_fm2t_rows_dev: model is not FM_TWOTOWER");
    PG_REQUIRE(n_req <= 65535, "pg_rank_fm2t_rows_dev: at most 65535 requests per call");
    if (n_items == 0 || n_req == 0) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    return pg::rank_fm2t_rows_dev_locked(ctx, m, fs, item_field_cols, d_user_vecs, d_user_field_ids, d_cand_rows, d_req_offsets,
                                         n_req, n_items, d_out_scores);
}

// host-buffer form of pg_rank_fm2t_rows_dev: what an IAlgorithm.Run of the EasyRec flavour passes — item ids resolved
// to rows, the per-item "context features" read from the device-resident columns instead of being boxed per request
int pg_rank_fm2t_rows(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                      const float* user_vecs, const int32_t* user_field_ids, const uint32_t* cand_rows,
                      const uint32_t* req_offsets, uint32_t n_req, float* out_scores) {
    PG_REQUIRE(ctx && m && fs && item_field_cols && req_offsets, "pg_rank_fm2t_rows: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_rank_fm2t_rows: model is not FM_TWOTOWER");
    const pg::HostIn in[] = {{user_vecs, false, m->d_user, 4}, {user_field_ids, false, m->nuf, 4}, {cand_rows, true, 1, 4},
                             {nullptr, true, m->nif, 4, false}};      // the item field ids, gathered below
    return pg::rank_from_host(
        "pg_rank_fm2t_rows", ctx, m, nullptr, in, user_field_ids, req_offsets, n_req, out_scores, pg::no_check,
        [&](void* const* d, const uint32_t* d_off, uint32_t n_items, float* d_scores) {
            int rc;
            if ((rc = pg::features_gather_i32_locked(ctx, fs, item_field_cols, m->nif, (const uint32_t*)d[2], n_items, (int32_t*)d[3],
                                                     "pg_rank_fm2t_rows")))
                return rc;
            return pg::rank_fm2t_dev_locked(ctx, m, (const float*)d[0], (const int32_t*)d[1], (const int32_t*)d[3], d_off, n_req, n_items,
                                            d_scores);
        });
}

int pg_rank_fm2t(pg_ctx* ctx, const pg_model* m, const float* user_vecs, const int32_t* user_field_ids,
                 const int32_t* item_field_ids, const uint32_t* req_offsets, uint32_t n_req,
                 float* out_scores) {
    PG_REQUIRE(ctx && m && req_offsets, "pg_rank_fm2t: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_rank_fm2t: model is not FM_TWOTOWER");
    const pg::HostIn in[] = {{user_vecs, false, m->d_user, 4}, {user_field_ids, false, m->nuf, 4}, {item_field_ids, true, m->nif, 4}};
    return pg::rank_from_host(
        "pg_rank_fm2t", ctx, m, nullptr, in, user_field_ids, req_offsets, n_req, out_scores,
        [&](uint32_t n_items) -> int {
            for (size_t i = 0; i < (size_t)n_items * m->nif; ++i)
                PG_REQUIRE(item_field_ids[i] >= 0 && (uint32_t)item_field_ids[i] < m->vocab,
                           "pg_rank_fm2t: item field id %d outside vocab %u", item_field_ids[i], m->vocab);
            return PG_OK;
        },
        [&](void* const* d, const uint32_t* d_off, uint32_t n_items, float* d_scores) {
            return pg::rank_fm2t_dev_locked(ctx, m, (const float*)d[0], (const int32_t*)d[1], (const int32_t*)d[2], d_off, n_req, n_items,
                                            d_scores);
        });
}

int pg_fm2t_item_rows_build(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                            pg_item_rows** out) {
    PG_REQUIRE(ctx && m && fs && item_field_cols && out, "pg_fm2t_item_rows_build: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER, "pg_fm2t_item_rows_build: model is not FM_TWOTOWER");
    PG_REQUIRE(m->nif <= 16 && m->nif * m->k == (uint32_t)pg::kDIN, "pg_fm2t_item_rows_build: unsupported item side (%u fields x %u)", m->nif, m->k);
    PG_REQUIRE(fs->rows < 0xFFFFFFFEull, "pg_fm2t_item_rows_build: too many rows");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    pg_item_rows* ir = new pg_item_rows();
    ir->m = m;
    ir->fs = fs;
    ir->rows = fs->rows;
    for (uint32_t f = 0; f < m->nif; ++f) ir->cols[f] = item_field_cols[f];
    const size_t bytes = (size_t)(fs->rows + 1) * pg::kItemRowFloats * 4;
    const hipError_t e = hipMalloc((void**)&ir->d, bytes);
    if (e != hipSuccess) {
        pg::set_error("pg_fm2t_item_rows_build: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        delete ir;
        return PG_ERR_NOMEM;
    }
    int rc;
    if ((rc = pg::item_rows_fill_locked(ctx, ir, 0, fs->rows + 1))) {       // + the defaults' record
        hipFree(ir->d);
        delete ir;
        return rc;
    }
    PG_HIP(hipStreamSynchronize(ctx->stream));
    *out = ir;
    return PG_OK;
}

int pg_fm2t_item_rows_update(pg_ctx* ctx, pg_item_rows* ir, uint64_t row0, uint64_t nrows) {
    PG_REQUIRE(ctx && ir, "pg_fm2t_item_rows_update: NULL argument");
    // (not row0 + nrows <= rows: the sum wraps for a huge row0, and the kernel would write far outside the records)
    PG_REQUIRE(row0 <= ir->rows && nrows <= ir->rows - row0, "pg_fm2t_item_rows_update: rows %llu + %llu outside the store's %llu",
               (unsigned long long)row0, (unsigned long long)nrows, (unsigned long long)ir->rows);
    std::lock_guard<std::mutex> g(ctx->mu);
    int rc;
    if ((rc = pg::item_rows_fill_locked(ctx, ir, row0, nrows))) return rc;
    if ((rc = pg::item_rows_fill_locked(ctx, ir, ir->rows, 1))) return rc;     // the defaults may have changed with the column
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_fm2t_item_rows_destroy(pg_ctx* ctx, pg_item_rows* ir) {
    PG_REQUIRE(ctx, "pg_fm2t_item_rows_destroy: NULL context");
    if (!ir) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipStreamSynchronize(ctx->stream));
    if (ir->d) PG_HIP(hipFree(ir->d));
    delete ir;
    return PG_OK;
}

int pg_rank_fm2t_irows_dev(pg_ctx* ctx, const pg_model* m, const pg_item_rows* ir, const float* d_user_vecs,
                           const int32_t* d_user_field_ids, const uint32_t* d_cand_rows, const uint32_t* d_req_offsets,
                           uint32_t n_req, uint32_t n_items, float* d_out_scores) {
    PG_REQUIRE(ctx && m && ir && d_user_vecs && d_user_field_ids && d_cand_rows && d_req_offsets && d_out_scores,
               "pg_rank_fm2t_irows_dev: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER && ir->m == m, "pg_rank_fm2t_irows_dev: the item records belong to another model");
    PG_REQUIRE(n_req <= 65535, "pg_rank_fm2t_irows_dev: at most 65535 requests per call");
    if (n_items == 0 || n_req == 0) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    return pg::rank_fm2t_irows_dev_locked(ctx, m, ir, d_user_vecs, d_user_field_ids, d_cand_rows, d_req_offsets, n_req, n_items, d_out_scores);
}

int pg_rank_fm2t_irows(pg_ctx* ctx, const pg_model* m, const pg_item_rows* ir, const float* user_vecs,
                       const int32_t* user_field_ids, const uint32_t* cand_rows, const uint32_t* req_offsets, uint32_t n_req,
                       float* out_scores) {
    PG_REQUIRE(ctx && m && ir && req_offsets, "pg_rank_fm2t_irows: NULL argument");
    PG_REQUIRE(m->kind == PG_MODEL_FM_TWOTOWER && ir->m == m, "pg_rank_fm2t_irows: the item records belong to another model");
    const pg::HostIn in[] = {{user_vecs, false, m->d_user, 4}, {user_field_ids, false, m->nuf, 4}, {cand_rows, true, 1, 4}};
    return pg::rank_from_host(
        "pg_rank_fm2t_irows", ctx, m, nullptr, in, user_field_ids, req_offsets, n_req, out_scores, pg::no_check,
        [&](void* const* d, const uint32_t* d_off, uint32_t n_items, float* d_scores) {
            return pg::rank_fm2t_irows_dev_locked(ctx, m, ir, (const float*)d[0], (const int32_t*)d[1], (const uint32_t*)d[2], d_off, n_req,
                                                  n_items, d_scores);
        });
}

}  // extern "C"
