// hot.hip — list recall over an HBM hot table: UserGroupHotRecall, UserGlobalHotRecall and UserTopicRecall as
// one primitive with three modes.  A request names triggers (the user's trigger ids, "-1" for the global list, topics); their
// stored lists are concatenated, scored, ordered by score or left in stored order, and cut to k.
//
// The reference: module/user_group_hot_recall_hologres_dao.go:47-140, module/user_global_hot_recall_hologres_dao.go:50-149,
// module/user_topic_mysql_dao.go:58-138.  hot_host.hpp states the answer; this file holds the table and the kernel.
//
// Storage: a CSR over dense trigger indices — offsets uint64[n_triggers + 1] (a host copy beside the device's: every request is
// validated and sized on the host), item rows uint32, scores fp64, a source byte per entry.
//
// One workgroup of 1024 lanes serves one request in one launch.  The lanes below the trigger count read their trigger's offsets;
// a block scan of the contributed lengths gives every trigger its base position.  Waves take the triggers round-robin, lanes
// stride a list.  A request whose answer is the stored order (TOPIC; GLOBAL with n <= k) is written straight from that gather.
// Otherwise every entry becomes a 16-byte record (the descending key of its score, position << 40 | entry index) — in LDS when
// the padded count is at most 8192, in the request's slice of kSlotHot above — ordered by cf_sort.hpp's bitonic sort; the
// first min(k, n) records find their row, score and source again through the entry index.
#include "block_rank.hpp"
#include "cf_sort.hpp"
#include "hot_host.hpp"

struct pg_hottable {
    // recalls share this lock while they enqueue, the uploads take it exclusively.  Lock order: ctx->mu, the item table, then this.
    mutable std::shared_mutex rw;
    const pg_table* t = nullptr;
    uint64_t gen = 0;              // t->generation at create: a recall on another generation is refused
    uint64_t rows = 0;
    uint32_t n_triggers = 0;
    std::vector<uint64_t> h_off;   // [n_triggers + 1]: the device offsets' host copy
    uint64_t* d_off = nullptr;
    uint32_t* d_rows = nullptr;    // [cap], `pairs` used
    double* d_sc = nullptr;
    uint8_t* d_src = nullptr;
    uint64_t pairs = 0, cap = 0;
    uint32_t uploaded = 0;         // the next upload starts at or behind this trigger
};

namespace pg {
namespace {

static_assert(kHotMaxTriggers <= kCfThreads && kHotLdsRecords == kCfSortChunk && kHotMaxQueries == (uint32_t)kMaxQueries,
              "the host statement's limits are the kernel's");
// LDS: the sort's records (kCfSortChunk x 16 B = 128 KiB) from the start, behind them the staged triggers — begin u64, base u32,
// len u32 [kHotMaxTriggers] — and the scan's wave sums.  132 KiB: one workgroup per CU.
constexpr size_t kHotStageAt = (size_t)kCfSortChunk * 16;
constexpr size_t kHotWordsAt = kHotStageAt + (size_t)kHotMaxTriggers * 16;
constexpr size_t kHotLds = kHotWordsAt + (kCfThreads / kWave) * 4;
static_assert(kHotStageAt % 16 == 0 && kHotLds <= 160 * 1024, "one workgroup's LDS");
constexpr unsigned long long kHotEntryMask = (1ull << 40) - 1;

struct HotArgs {
    const uint64_t* off;           // [n_triggers + 1]
    const uint32_t* rows;
    const double* sc;
    const uint8_t* src;
    uint32_t n_triggers;
    uint64_t row_offset;
    int mode;
    // staged by the call (hot_host.hpp's HotStage): [nq + 1] trigger offsets, [nq] the host's n, [nq] the request's first record
    // in `slab` (kHotNone: its records live in LDS, or it has none), [total] trigger ids, [total] quotas (PG_HOT_TOPIC only)
    const uint32_t* st_off;
    const uint32_t* st_n;
    const uint32_t* st_slab;
    const uint32_t* st_trig;
    const uint32_t* st_quota;
    const uint64_t* seed;          // [nq] or NULL
    ulonglong2* slab;
    uint32_t k;
    uint64_t* out_rows;            // [nq][k]
    double* out_scores;
    uint8_t* out_source;           // or NULL
    uint32_t* out_count;           // [nq] or NULL
};

// entry e at position p -> slot o of the outputs
__device__ __forceinline__ void hot_write(const HotArgs& a, size_t o, uint64_t e, uint32_t p, unsigned long long seed) {
    const uint8_t s = a.src[e];
    a.out_rows[o] = a.row_offset + a.rows[e];
    a.out_scores[o] = hot_entry_score(a.mode, s, a.sc[e], seed, p);
    if (a.out_source) a.out_source[o] = s & kHotSourceMask;
}

// Request q = blockIdx.x.
__global__ __launch_bounds__(kCfThreads) void hot_recall_kernel(HotArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hot_lds[];
    ulonglong2* s_rec = reinterpret_cast<ulonglong2*>(hot_lds);
    uint64_t* tb_begin = reinterpret_cast<uint64_t*>(hot_lds + kHotStageAt);
    uint32_t* tb_base = reinterpret_cast<uint32_t*>(tb_begin + kHotMaxTriggers);
    uint32_t* tb_len = tb_base + kHotMaxTriggers;
    uint32_t* ws = reinterpret_cast<uint32_t*>(hot_lds + kHotWordsAt);
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t t0 = a.st_off[q];
    const uint32_t nt = min(a.st_off[q + 1] - t0, kHotMaxTriggers);
    const unsigned long long seed = a.seed ? a.seed[q] : 0ull;
    // ---- stage the triggers: a trigger of UINT32_MAX or >= n_triggers contributes nothing ----
    uint64_t begin = 0;
    uint32_t len = 0;
    if (tid < nt) {
        const uint32_t t = a.st_trig[t0 + tid];
        if (t < a.n_triggers) {
            begin = a.off[t];
            const uint64_t l = a.off[t + 1] - begin;
            len = l < kHotMaxEntries ? (uint32_t)l : kHotMaxEntries;
            if (a.mode == PG_HOT_TOPIC) len = min(len, a.st_quota[t0 + tid]);
        }
    }
    uint32_t n;
    const uint32_t base = block_excl_scan<kCfThreads / kWave, uint32_t>(len, ws, &n);
    if (tid < nt) {
        tb_begin[tid] = begin;
        tb_base[tid] = base;
        tb_len[tid] = len;
    }
    __syncthreads();
    // (the host sized this request from the same offsets; its n bounds every position written)
    n = min(n, a.st_n[q]);
    const uint32_t kept = min(n, a.k);
    const size_t out0 = (size_t)q * a.k;
    if (!hot_is_sorted(a.mode, n, a.k)) {
        // ---- the stored order IS the answer: position p goes to slot p ----
        for (uint32_t j = wave; j < nt; j += kCfThreads / kWave) {
            const uint64_t b = tb_begin[j];
            const uint32_t pb = tb_base[j], l = tb_len[j];
            for (uint32_t i = lane; i < l; i += kWave) {
                const uint32_t p = pb + i;
                if (p < kept) hot_write(a, out0 + p, b + i, p, seed);
            }
        }
    } else if (n) {
        // ---- records, their order, the cut ----
        const uint32_t slab_at = a.st_slab[q];
        const uint32_t np2 = hot_next_pow2(n);
        ulonglong2* rec = slab_at == kHotNone ? s_rec : a.slab + slab_at;
        for (uint32_t j = wave; j < nt; j += kCfThreads / kWave) {
            const uint64_t b = tb_begin[j];
            const uint32_t pb = tb_base[j], l = tb_len[j];
            for (uint32_t i = lane; i < l; i += kWave) {
                const uint32_t p = pb + i;
                if (p >= n) continue;
                const uint64_t e = b + i;
                const double sc = hot_entry_score(a.mode, a.src[e], a.sc[e], seed, p);
                rec[p] = make_ulonglong2(hot_key(hot_bits(sc)), ((unsigned long long)p << 40) | e);
            }
        }
        for (uint32_t i = n + tid; i < np2; i += kCfThreads) rec[i] = make_ulonglong2(~0ull, ~0ull);
        __syncthreads();
        if (slab_at == kHotNone) cf_sort_lds(s_rec, s_rec, 0, np2, 2, np2);      // (np2 <= kCfSortChunk: ordered where it lies)
        else cf_sort(rec, s_rec, np2);
        for (uint32_t j = tid; j < kept; j += kCfThreads) {
            const ulonglong2 r = rec[j];
            hot_write(a, out0 + j, r.y & kHotEntryMask, (uint32_t)(r.y >> 40), seed);
        }
    }
    for (uint32_t j = kept + tid; j < a.k; j += kCfThreads) {
        a.out_rows[out0 + j] = ~0ull;
        a.out_scores[out0 + j] = -__builtin_inf();
        if (a.out_source) a.out_source[out0 + j] = kHotPadSource;
    }
    if (tid == 0 && a.out_count) a.out_count[q] = kept;
}

int hot_refuse(const HotRefusal& r) {
    set_error("%s", r.msg);
    return r.code;
}

int hot_stale_check(const char* who, const pg_hottable* h) {
    const uint64_t gen = h->t->generation.load(std::memory_order_relaxed);
    PG_REQUIRE(gen == h->gen, "%s: the hot table describes generation %llu of its item table, which is at generation %llu (stale)", who,
               (unsigned long long)h->gen, (unsigned long long)gen);
    return PG_OK;
}

// One launch over nq checked requests into device outputs.  Caller holds ctx->mu, the item table's shared lock and the hot
// table's; nothing synchronises (a growing kSlotHot does).  Every request is sized from the table's host offsets first: a
// refusal enqueues nothing.
int hot_recall_locked(const char* who, pg_ctx* ctx, const pg_hottable* h, int mode, const uint32_t* triggers, const double* values,
                      const uint32_t* off, const uint64_t* d_seed, uint32_t nq, uint32_t k, uint64_t* d_out_rows, double* d_out_scores,
                      uint8_t* d_out_source, uint32_t* d_out_count) {
    int rc;
    HotStage st;
    HotRefusal r;
    if (!hot_stage_build(who, mode, h->n_triggers, h->h_off.data(), triggers, values, off, nq, k, &st, &r)) return hot_refuse(r);
    uint32_t* d_st; ulonglong2* d_slab;
    if ((rc = scratch_carve(ctx, kSlotHot, [&](Carve& c) {
            d_st = c.take<uint32_t>(st.words.size());
            d_slab = c.take<ulonglong2>(st.slab_records);
        }))) return rc;
    // (pageable memory: the runtime has read the words when the copy call returns, as with rtu2i.hip's staged offsets)
    PG_HIP(hipMemcpyAsync(d_st, st.words.data(), st.words.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HotArgs a;
    a.off = h->d_off;
    a.rows = h->d_rows;
    a.sc = h->d_sc;
    a.src = h->d_src;
    a.n_triggers = h->n_triggers;
    a.row_offset = h->t->row_offset;
    a.mode = mode;
    a.st_off = d_st;
    a.st_n = d_st + st.n_at;
    a.st_slab = d_st + st.slab_at;
    a.st_trig = d_st + st.trig_at;
    a.st_quota = d_st + st.quota_at;
    a.seed = d_seed;
    a.slab = d_slab;
    a.k = k;
    a.out_rows = d_out_rows;
    a.out_scores = d_out_scores;
    a.out_source = d_out_source;
    a.out_count = d_out_count;
    if ((rc = ensure_dyn_lds(ctx, (const void*)hot_recall_kernel, kHotLds))) return rc;
    hot_recall_kernel<<<nq, kCfThreads, kHotLds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int hot_entry(const char* who, pg_ctx* ctx, const pg_hottable* h, int mode, const uint32_t* triggers, const double* values, const uint32_t* off,
              const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* rows, double* scores, uint8_t* source, uint32_t* count, bool host) {
    int rc;
    PG_REQUIRE(ctx && h, "%s: NULL argument", who);
    HotRefusal r;
    if (!hot_check_args(who, mode, triggers, values, off, nq, k, rows, scores, &r)) return hot_refuse(r);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    TableRead tr(h->t->rw);
    std::shared_lock<std::shared_mutex> sr(h->rw);
    if ((rc = hot_stale_check(who, h))) return rc;
    if (!host) return hot_recall_locked(who, ctx, h, mode, triggers, values, off, seed, nq, k, rows, scores, source, count);
    // host buffers: the seeds in, the answer out, through the staging slot
    const size_t nk = (size_t)nq * k;
    uint64_t *d_seed, *d_rows; double* d_sc; uint8_t* d_src; uint32_t* d_cnt;
    if ((rc = scratch_carve(ctx, kSlotStaging, [&](Carve& c) {
            d_seed = c.take<uint64_t>(seed ? nq : 0);
            d_rows = c.take<uint64_t>(nk);
            d_sc = c.take<double>(nk);
            d_src = c.take<uint8_t>(nk);
            d_cnt = c.take<uint32_t>(nq);
        }))) return rc;
    if (seed) PG_HIP(hipMemcpyAsync(d_seed, seed, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = hot_recall_locked(who, ctx, h, mode, triggers, values, off, seed ? d_seed : nullptr, nq, k, d_rows, d_sc, d_src, d_cnt))) return rc;
    PG_HIP(hipMemcpyAsync(rows, d_rows, nk * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(scores, d_sc, nk * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (source) PG_HIP(hipMemcpyAsync(source, d_src, nk, hipMemcpyDeviceToHost, ctx->stream));
    if (count) PG_HIP(hipMemcpyAsync(count, d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

void hot_free_arrays(pg_hottable* h) {
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_rows) (void)hipFree(h->d_rows);
    if (h->d_sc) (void)hipFree(h->d_sc);
    if (h->d_src) (void)hipFree(h->d_src);
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_hottable_create(pg_ctx* ctx, const pg_table* t, uint32_t n_triggers, pg_hottable** out) {
    const char* who = "pg_hottable_create";
    PG_REQUIRE(ctx && t && out, "%s: NULL argument", who);
    PG_REQUIRE(t->rows >= 1 && t->rows <= 0xFFFFFFFFull, "%s: a table of %llu rows (1 .. 2^32 - 1)", who, (unsigned long long)t->rows);
    PG_REQUIRE(n_triggers >= 1 && n_triggers < 0xFFFFFFFFu, "%s: n_triggers=%u (1 .. 2^32 - 2)", who, n_triggers);
    PG_REQUIRE(!t->d_row_map, "%s: a filtered view has no hot table (its rows are not the source's)", who);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    pg::TableRead tr(t->rw);
    std::unique_ptr<pg_hottable> h(new pg_hottable());
    h->t = t;
    h->gen = t->generation.load(std::memory_order_relaxed);
    h->rows = t->rows;
    h->n_triggers = n_triggers;
    h->h_off.assign((size_t)n_triggers + 1, 0);
    const size_t bytes = ((size_t)n_triggers + 1) * 8;
    if (hipMalloc((void**)&h->d_off, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->d_off = nullptr;
        pg::set_error("%s: hipMalloc(%.1f MB) failed", who, (double)bytes / 1e6);
        return PG_ERR_NOMEM;
    }
    // a trigger whose list was never uploaded has an empty one
    if (hipMemsetAsync(h->d_off, 0, bytes, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(h->d_off);
        pg::set_error("%s: clearing the offsets failed", who);
        return PG_ERR_DEVICE;
    }
    *out = h.release();
    return PG_OK;
}

int pg_hottable_upload(pg_ctx* ctx, pg_hottable* h, uint32_t trig0, uint32_t ntrig, const uint64_t* offsets, const uint32_t* item_rows,
                       const double* scores, const uint8_t* source) {
    const char* who = "pg_hottable_upload";
    PG_REQUIRE(ctx && h && offsets, "%s: NULL argument", who);
    PG_REQUIRE(trig0 <= h->n_triggers && ntrig <= h->n_triggers - trig0, "%s: triggers [%u, %llu) outside the table's %u", who, trig0,
               (unsigned long long)trig0 + ntrig, h->n_triggers);
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> sw(h->rw);
    PG_REQUIRE(trig0 >= h->uploaded, "%s: trigger %u after triggers up to %u were uploaded (triggers arrive in ascending order)", who, trig0,
               h->uploaded);
    // every refusal comes before the first change: a refused upload leaves the table as it was
    pg::HotRefusal r;
    if (!pg::hot_validate_lists(who, trig0, ntrig, offsets, item_rows, scores, source, h->rows, h->pairs, &r)) return pg::hot_refuse(r);
    if (ntrig == 0) return PG_OK;
    const uint64_t total = offsets[ntrig] - offsets[0];
    PG_HIP(hipSetDevice(ctx->device));
    // (recalls are enqueue-only: whatever any context has enqueued over these arrays ends before they change)
    PG_HIP(hipDeviceSynchronize());
    if (h->pairs + total > h->cap) {
        const uint64_t cap = std::max<uint64_t>(h->pairs + total, h->cap + h->cap / 2);
        uint32_t* nr = nullptr;
        double* ns = nullptr;
        uint8_t* nb = nullptr;
        if (hipMalloc((void**)&nr, cap * 4) != hipSuccess || hipMalloc((void**)&ns, cap * 8) != hipSuccess ||
            hipMalloc((void**)&nb, cap) != hipSuccess) {
            (void)hipGetLastError();
            if (nr) (void)hipFree(nr);
            if (ns) (void)hipFree(ns);
            pg::set_error("%s: hipMalloc(%.1f MB) failed", who, (double)(cap * 13) / 1e6);
            return PG_ERR_NOMEM;
        }
        if (h->pairs) {
            PG_HIP(hipMemcpyAsync(nr, h->d_rows, h->pairs * 4, hipMemcpyDeviceToDevice, ctx->stream));
            PG_HIP(hipMemcpyAsync(ns, h->d_sc, h->pairs * 8, hipMemcpyDeviceToDevice, ctx->stream));
            PG_HIP(hipMemcpyAsync(nb, h->d_src, h->pairs, hipMemcpyDeviceToDevice, ctx->stream));
            PG_HIP(hipStreamSynchronize(ctx->stream));
        }
        if (h->d_rows) (void)hipFree(h->d_rows);
        if (h->d_sc) (void)hipFree(h->d_sc);
        if (h->d_src) (void)hipFree(h->d_src);
        h->d_rows = nr;
        h->d_sc = ns;
        h->d_src = nb;
        h->cap = cap;
    }
    // the new offsets from trig0 on: the uploaded triggers' lists, then every later trigger at the new total (the triggers between
    // the last upload and trig0 already end at the old total: their lists stay empty).  The host copy takes them only once the
    // device holds them, together with `pairs` and `uploaded`.
    std::vector<uint64_t> noff((size_t)h->n_triggers + 1 - trig0, h->pairs + total);
    for (uint32_t i = 0; i < ntrig; ++i) noff[i] = h->pairs + (offsets[i] - offsets[0]);
    PG_HIP(hipMemcpyAsync(h->d_off + trig0, noff.data(), noff.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (total) {
        PG_HIP(hipMemcpyAsync(h->d_rows + h->pairs, item_rows + offsets[0], total * 4, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(h->d_sc + h->pairs, scores + offsets[0], total * 8, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(h->d_src + h->pairs, source + offsets[0], total, hipMemcpyHostToDevice, ctx->stream));
    }
    PG_HIP(hipStreamSynchronize(ctx->stream));
    std::copy(noff.begin(), noff.end(), h->h_off.begin() + trig0);
    h->pairs += total;
    h->uploaded = trig0 + ntrig;
    return PG_OK;
}

int pg_hottable_info(const pg_hottable* h, uint64_t* rows, uint32_t* n_triggers, uint64_t* pairs, uint32_t* triggers_uploaded,
                     uint64_t* generation) {
    PG_REQUIRE(h, "pg_hottable_info: table is NULL");
    std::shared_lock<std::shared_mutex> sr(h->rw);
    if (rows) *rows = h->rows;
    if (n_triggers) *n_triggers = h->n_triggers;
    if (pairs) *pairs = h->pairs;
    if (triggers_uploaded) *triggers_uploaded = h->uploaded;
    if (generation) *generation = h->gen;
    return PG_OK;
}

int pg_hottable_destroy(pg_ctx* ctx, pg_hottable* h) {
    PG_REQUIRE(ctx, "pg_hottable_destroy: ctx is NULL");
    if (!h) return PG_OK;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        std::unique_lock<std::shared_mutex> sw(h->rw);
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipDeviceSynchronize());
        pg::hot_free_arrays(h);
    }
    delete h;
    return PG_OK;
}

int pg_hot_recall_dev(pg_ctx* ctx, const pg_hottable* h, int mode, const uint32_t* triggers, const double* trigger_value,
                      const uint32_t* trigger_offsets, const uint64_t* d_seed, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                      double* d_out_scores, uint8_t* d_out_source, uint32_t* d_out_count) {
    return pg::hot_entry("pg_hot_recall_dev", ctx, h, mode, triggers, trigger_value, trigger_offsets, d_seed, nq, k, d_out_rows, d_out_scores,
                         d_out_source, d_out_count, false);
}

int pg_hot_recall(pg_ctx* ctx, const pg_hottable* h, int mode, const uint32_t* triggers, const double* trigger_value,
                  const uint32_t* trigger_offsets, const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows, double* out_scores,
                  uint8_t* out_source, uint32_t* out_count) {
    return pg::hot_entry("pg_hot_recall", ctx, h, mode, triggers, trigger_value, trigger_offsets, seed, nq, k, out_rows, out_scores, out_source,
                         out_count, true);
}

int pg_hot_recall_host(uint64_t rows, uint64_t row_offset, uint32_t n_triggers, const uint64_t* offsets, const uint32_t* item_rows,
                       const double* scores, const uint8_t* source, int mode, const uint32_t* triggers, const double* trigger_value,
                       const uint32_t* trigger_offsets, const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows, double* out_scores,
                       uint8_t* out_source, uint32_t* out_count) {
    const char* who = "pg_hot_recall_host";
    PG_REQUIRE(offsets, "%s: NULL argument", who);
    PG_REQUIRE(rows >= 1 && rows <= 0xFFFFFFFFull && n_triggers >= 1 && n_triggers < 0xFFFFFFFFu, "%s: rows=%llu (1 .. 2^32 - 1), n_triggers=%u (1 .. 2^32 - 2)",
               who, (unsigned long long)rows, n_triggers);
    pg::HotRefusal r;
    if (!pg::hot_check_args(who, mode, triggers, trigger_value, trigger_offsets, nq, k, out_rows, out_scores, &r)) return pg::hot_refuse(r);
    // the CSR is held to what the upload accepts
    if (!pg::hot_validate_lists(who, 0, n_triggers, offsets, item_rows, scores, source, rows, 0, &r)) return pg::hot_refuse(r);
    const pg::HotTableHost t{rows, row_offset, n_triggers, offsets, item_rows, scores, source};
    if (!pg::hot_recall_host(who, t, mode, triggers, trigger_value, trigger_offsets, seed, nq, k, out_rows, out_scores, out_source, out_count, &r))
        return pg::hot_refuse(r);
    return PG_OK;
}

}  // extern "C"
