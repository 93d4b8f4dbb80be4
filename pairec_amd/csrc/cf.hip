// cf.hip — collaborative-filter recall (U2I2I) over an HBM similarity table.
//
// UserCollaborativeFilterRecall (service/recall/user_collaborative_filter_recall.go:31-80) expands a user's trigger items into
// their similar-item lists (module/user_collaborative_hologres_dao.go:58-216: four goroutines of SELECT ... WHERE item_id IN),
// multiplies every similarity by the trigger's preference (:179-192), sums the products per distinct item in float64
// (module/user_collaborative_dao.go:38-51), optionally divides by the largest sum (:61-65), sorts descending and cuts to
// RecallCount.  Here the lists are CSR over the local rows of an item table and one workgroup serves one request: a sparse
// gather, a keyed fp64 reduction in an open-addressed table, and an ordered cut.
//
// Storage: offsets uint64[rows + 1], neighbours uint32[pairs] (local rows of the item table), similarities float[pairs].  The
// reference parses similarities from text as float64; here they are stored fp32, like every table of this engine, and widened
// exactly when used (term = (double)sim * prefer: one rounding).
//
// Determinism without floating-point atomics: triggers are processed one after the other with a barrier between them, a
// trigger's list is spread over the lanes, and a list holds no neighbour twice (pg_simtable_upload refuses it), so no two
// lanes of one trigger touch one slot.  Every item's additions happen in trigger order with a plain read-modify-write; only
// the slot's uint32 key is claimed by compare-and-swap.
//
// RealTimeU2IRecall's expansion (pg_rtu2i_expand, pg_rtu2i_recall) is the same kernel with another reduction: an
// item keeps the LARGEST of its terms — the first, replaced only by a larger one — and nothing is normalised
// (module/realtime_user2item_hologres_dao.go:203-204: a descending sort, then uniqItems).  Its triggers may come from rtu2i.hip's
// trigger kernel: lists at a fixed stride with a device count per request (CfTrigDev), read without a host round trip.
//
// The accumulation, the sort, the cut and the padding are in cf_kernel.hpp: x2i.hip runs the same code behind
// its first hop.
#include "cf_kernel.hpp"

#include <cmath>
#include <functional>

struct pg_simtable {
    // recalls share this lock, pg_simtable_upload takes it exclusively.  Lock order: ctx->mu, the item table, then this.
    mutable std::shared_mutex rw;
    const pg_table* t = nullptr;
    uint64_t gen = 0;              // t->generation at create: a recall on another generation is refused
    uint64_t rows = 0;
    uint64_t* d_off = nullptr;     // [rows + 1]
    uint32_t* d_nbr = nullptr;     // [cap], pairs used
    float* d_sim = nullptr;
    uint64_t pairs = 0, cap = 0;
    uint64_t rows_uploaded = 0;    // the next upload starts at or behind this row
};

namespace pg {
namespace {

// LDS tier: 12288 slots of (fp64 accumulator, uint32 key) in two planes = 144 KiB; load factor <= 0.5 serves 6144 pairs.  The
// planes keep the 8-byte accumulators of neighbouring slots on neighbouring bank pairs and the keys' probes (4-byte reads,
// 32-bank modulus) apart from them; a 16-byte record per slot would hold a third less.
constexpr uint32_t kCfLdsSlots = 12288;
constexpr uint32_t kCfLdsMaxPairs = kCfLdsSlots / 2;
constexpr size_t kCfTableBytes = (size_t)kCfLdsSlots * 12;
static_assert((size_t)kCfSortChunk * 16 <= kCfTableBytes, "the sort reuses the table's LDS");
constexpr size_t kCfLds = kCfTableBytes + kCfMaxTriggers * (8 + 8 + 4) + 64;
static_assert(kCfLds <= 160 * 1024, "one workgroup's LDS");

// Request q = blockIdx.x.  trigger_prefer must be finite (the host entry point checks it).
template <bool kMax>
__global__ __launch_bounds__(kCfThreads) void cf_recall_kernel(CfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cf_lds[];
    uint64_t* tb_begin = reinterpret_cast<uint64_t*>(cf_lds + kCfTableBytes);
    double* tb_pref = reinterpret_cast<double*>(tb_begin + kCfMaxTriggers);
    uint32_t* tb_len = reinterpret_cast<uint32_t*>(tb_pref + kCfMaxTriggers);
    unsigned long long* max_bits = reinterpret_cast<unsigned long long*>(tb_len + kCfMaxTriggers);
    uint32_t* n_pairs = reinterpret_cast<uint32_t*>(max_bits + 1);
    uint32_t* n_items = n_pairs + 1;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t t0 = a.trig_off ? a.trig_off[q] : q * a.trig_stride;
    const uint32_t nt = min(a.trig_off ? a.trig_off[q + 1] - t0 : min(a.trig_cnt[q], a.trig_stride), kCfMaxTriggers);
    if (tid == 0) {
        *max_bits = 0;
        *n_pairs = 0;
        *n_items = 0;
    }
    __syncthreads();
    if (tid < nt) {
        // a trigger of UINT32_MAX or >= rows contributes nothing: the id the reference's SQL does not return
        const uint32_t r = a.trig[t0 + tid];
        uint64_t b = 0;
        uint32_t len = 0;
        if (r < a.rows) {
            b = a.off[r];
            len = (uint32_t)(a.off[r + 1] - b);
        }
        tb_begin[tid] = b;
        tb_len[tid] = len;
        tb_pref[tid] = a.pref[t0 + tid];
        if (len) atomicAdd(n_pairs, len);
    }
    __syncthreads();
    const uint32_t pairs = *n_pairs;
    if (pairs > kCfMaxPairs) {
        if (tid == 0) {
            atomicMin(a.status, q);
            a.out_count[q] = 0;
        }
        cf_pad(a, q, 0);
        return;
    }
    ulonglong2* cand = a.cand + (size_t)q * a.cand_cap;
    // the tier is the kernel's own decision, from the lists' offsets: no host read-back before the launch
    if (pairs <= min(a.lds_max_pairs, kCfLdsMaxPairs)) {
        double* acc = reinterpret_cast<double*>(cf_lds);
        uint32_t* keys = reinterpret_cast<uint32_t*>(cf_lds + (size_t)kCfLdsSlots * 8);
        cf_accumulate<true, kMax>(a, keys, acc, kCfLdsSlots, nt, tb_begin, tb_pref, tb_len, cand, n_items, max_bits);
    } else {
        uint32_t slots = kCfThreads;
        while (slots < 2 * pairs) slots <<= 1;
        slots = min(slots, a.gslots);                    // (distinct items <= min(pairs, rows) <= gslots / 2 either way)
        cf_accumulate<false, kMax>(a, a.gkeys + (size_t)q * a.gslots, a.gacc + (size_t)q * a.gslots, slots, nt, tb_begin, tb_pref, tb_len,
                                   cand, n_items, max_bits);
    }
    cf_finish(a, q, cand, n_items, max_bits, cf_lds);
}

// the arguments every form of the recall checks, in this order (dev_trig: the triggers are a CfTrigDev made by the call itself —
// no trigger arrays, no offsets)
int cf_check(const char* who, const pg_ctx* ctx, const pg_simtable* s, const void* trig, const void* pref, const uint32_t* off, uint32_t nq,
             uint32_t k, const pg_cf_opts* opts, const void* rows, const void* scores, uint32_t* nmax_out, bool dev_trig = false) {
    PG_REQUIRE(ctx && s && (off || dev_trig) && rows && scores, "%s: NULL argument", who);
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    if (k < 1 || k > kCfMaxDepth) {
        set_error("%s: k=%u unsupported (1..%u)", who, k, kCfMaxDepth);
        return PG_ERR_UNSUPPORTED;
    }
    for (uint32_t q = 0; q < nq && !dev_trig; ++q) {
        PG_REQUIRE(off[q + 1] >= off[q], "%s: trigger_offsets[%u] = %u is below trigger_offsets[%u] = %u", who, q + 1, off[q + 1], q, off[q]);
        if (off[q + 1] - off[q] > kCfMaxTriggers) {
            set_error("%s: request %u has %u triggers (at most %u per request)", who, q, off[q + 1] - off[q], kCfMaxTriggers);
            return PG_ERR_UNSUPPORTED;
        }
    }
    PG_REQUIRE(dev_trig || (trig && pref) || off[nq] == off[0], "%s: NULL argument", who);
    uint32_t nmax = 0;
    const uint32_t* xo = opts ? opts->excl_offsets : nullptr;
    if (xo) {
        for (uint32_t q = 0; q < nq; ++q) {
            PG_REQUIRE(xo[q + 1] >= xo[q], "%s: excl_offsets[%u] = %u is below excl_offsets[%u] = %u", who, q + 1, xo[q + 1], q, xo[q]);
            if (xo[q + 1] - xo[q] > kMaxExclude) {
                set_error("%s: request %u excludes %u ids (at most %u per request)", who, q, xo[q + 1] - xo[q], kMaxExclude);
                return PG_ERR_UNSUPPORTED;
            }
            nmax = std::max(nmax, xo[q + 1] - xo[q]);
        }
        PG_REQUIRE(opts->excl_rows || xo[nq] == xo[0], "%s: excl_rows is NULL", who);
        if ((uint64_t)k + nmax > kCfMaxDepth) {
            set_error("%s: k=%u plus the longest exclusion list of %u ids exceeds the depth of %u", who, k, nmax, kCfMaxDepth);
            return PG_ERR_UNSUPPORTED;
        }
    } else {
        PG_REQUIRE(!opts || !opts->excl_rows, "%s: excl_rows without excl_offsets", who);
    }
    *nmax_out = nmax;
    return PG_OK;
}

// The recall of nq requests whose triggers are device memory (indexed by the host offsets `off` as given) into device outputs
// [nq][k]; lists: host ids (staged here) or device ids, host offsets.  Caller holds ctx->mu, the item table's shared lock and
// the similarity table's; ends synchronised.  max_rule: pg_rtu2i_expand's reduction (no normalisation).  With `off` NULL the
// triggers are what make_trig describes: it is called once everything of this call is staged and its staging synchronised,
// right in front of the launch, so what it enqueues (the trigger kernel) and the expansion run back to back on the stream.
int cf_recall_locked(const char* who, pg_ctx* ctx, const pg_simtable* s, const uint32_t* d_trig, const double* d_pref, const uint32_t* off,
                     uint32_t nq, uint32_t k, int normalize, const uint64_t* excl, bool excl_on_host, const uint32_t* xoff, uint32_t nmax,
                     uint64_t* d_out_rows, double* d_out_scores, uint32_t* out_count, bool max_rule = false,
                     const std::function<int(CfTrigDev*)>& make_trig = nullptr) {
    int rc;
    const uint32_t rows_eff = (uint32_t)std::min<uint64_t>(kCfMaxPairs, s->rows);
    uint32_t gslots = kCfThreads, cand_cap = 1;
    while (gslots < 2 * rows_eff) gslots <<= 1;
    while (cand_cap < rows_eff) cand_cap <<= 1;
    const uint32_t kd = k + nmax;
    const uint32_t xtotal = nmax && excl_on_host ? xoff[nq] - xoff[0] : 0;
    uint32_t *d_status, *d_off, *d_xoff, *d_keys; uint64_t *d_list, *d_xrows; double *d_acc, *d_xsc; ulonglong2* d_cand; float *d_xidx, *d_oidx;
    if ((rc = scratch_carve(ctx, kSlotCf, [&](Carve& c) {
            d_status = c.take<uint32_t>(1 + (size_t)kMaxQueries);      // ONE region, copied out together: [0] the status word, [1 + q] request q's count
            d_off = c.take<uint32_t>(off ? (size_t)nq + 1 : 0);
            d_xoff = c.take<uint32_t>((size_t)nq + 1);
            d_list = c.take<uint64_t>(xtotal);
            d_keys = c.take<uint32_t>((size_t)nq * gslots);
            d_acc = c.take<double>((size_t)nq * gslots);
            d_cand = c.take<ulonglong2>((size_t)nq * cand_cap);
            d_xrows = c.take<uint64_t>(nmax ? (size_t)nq * kd : 0);
            d_xsc = c.take<double>(nmax ? (size_t)nq * kd : 0);
            d_xidx = c.take<float>(nmax ? (size_t)nq * kd : 0);
            d_oidx = c.take<float>(nmax ? (size_t)nq * k : 0);
        }))) return rc;
    uint32_t h_xoff[kMaxQueries + 1];
    PG_HIP(hipMemsetAsync(d_status, 0xFF, 4, ctx->stream));
    if (off) PG_HIP(hipMemcpyAsync(d_off, off, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (nmax) {
        for (uint32_t q = 0; q <= nq; ++q) h_xoff[q] = excl_on_host ? xoff[q] - xoff[0] : xoff[q];
        PG_HIP(hipMemcpyAsync(d_xoff, h_xoff, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        if (xtotal) PG_HIP(hipMemcpyAsync(d_list, excl + xoff[0], (size_t)xtotal * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    PG_HIP(hipStreamSynchronize(ctx->stream));           // (the staged offsets live on the callers' frames)
    CfTrigDev td;
    if (!off && (rc = make_trig(&td))) return rc;
    CfArgs a;
    a.off = s->d_off;
    a.nbr = s->d_nbr;
    a.sim = s->d_sim;
    a.rows = (uint32_t)s->rows;
    a.row_offset = s->t->row_offset;
    a.trig = off ? d_trig : td.d_rows;
    a.pref = off ? d_pref : td.d_weight;
    a.trig_off = off ? d_off : nullptr;
    a.trig_cnt = td.d_count;
    a.trig_stride = td.stride;
    a.lds_max_pairs = std::min(ctx->knobs.cf_lds_max_pairs, kCfLdsMaxPairs);
    a.gslots = gslots;
    a.gkeys = d_keys;
    a.gacc = d_acc;
    a.cand = d_cand;
    a.cand_cap = cand_cap;
    a.normalize = normalize;
    a.kd = kd;
    a.out_rows = nmax ? d_xrows : d_out_rows;
    a.out_scores = nmax ? d_xsc : d_out_scores;
    a.out_idx = nmax ? d_xidx : nullptr;
    a.out_count = d_status + 1;
    a.status = d_status;
    if (max_rule) {
        if ((rc = ensure_dyn_lds(ctx, (const void*)cf_recall_kernel<true>, kCfLds))) return rc;
        cf_recall_kernel<true><<<nq, kCfThreads, kCfLds, ctx->stream>>>(a);
    } else {
        if ((rc = ensure_dyn_lds(ctx, (const void*)cf_recall_kernel<false>, kCfLds))) return rc;
        cf_recall_kernel<false><<<nq, kCfThreads, kCfLds, ctx->stream>>>(a);
    }
    PG_HIP(hipGetLastError());
    if (nmax) {
        // the existing compaction on the row plane; its fp32 score plane carries each entry's index into the fp64 scores
        if ((rc = exclude_compact_locked(ctx, d_xrows, d_xidx, nq, kd, excl_on_host ? d_list : excl, d_xoff, k, 0.0f, d_out_rows, d_oidx,
                                         d_status + 1)))
            return rc;
        cf_gather_scores_kernel<<<dim3((k + 255) / 256, nq), 256, 0, ctx->stream>>>(d_xsc, d_oidx, d_status + 1, kd, k, d_out_scores);
        PG_HIP(hipGetLastError());
    }
    PG_HIP(hipMemcpyAsync(ctx->h_status, d_status, (1 + (size_t)nq) * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->h_status[0] != 0xFFFFFFFFu) {
        set_error("%s: request %u expands to more than %u (trigger, neighbour) pairs", who, ctx->h_status[0], kCfMaxPairs);
        return PG_ERR_UNSUPPORTED;
    }
    if (out_count) memcpy(out_count, ctx->h_status + 1, (size_t)nq * 4);
    return PG_OK;
}

int cf_entry(const char* who, pg_ctx* ctx, const pg_simtable* s, const uint32_t* trig, const double* pref, const uint32_t* off, uint32_t nq,
             uint32_t k, const pg_cf_opts* opts, uint64_t* rows, double* scores, uint32_t* out_count, bool host, bool max_rule = false) {
    int rc;
    uint32_t nmax = 0;
    if ((rc = cf_check(who, ctx, s, trig, pref, off, nq, k, opts, rows, scores, &nmax))) return rc;
    const uint32_t total = off[nq] - off[0];
    if (host)
        for (uint32_t i = 0; i < total; ++i)
            PG_REQUIRE(std::isfinite(pref[off[0] + i]), "%s: trigger_prefer[%u] is not finite", who, off[0] + i);
    const int normalize = max_rule ? 0 : opts ? opts->normalize : 1;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    TableRead tr(s->t->rw);
    std::shared_lock<std::shared_mutex> sr(s->rw);
    const uint64_t gen = s->t->generation.load(std::memory_order_relaxed);
    PG_REQUIRE(gen == s->gen, "%s: the similarity table describes generation %llu of its item table, which is at generation %llu (stale)",
               who, (unsigned long long)s->gen, (unsigned long long)gen);
    const uint64_t* excl = opts ? opts->excl_rows : nullptr;
    const uint32_t* xoff = opts ? opts->excl_offsets : nullptr;
    if (!host) return cf_recall_locked(who, ctx, s, trig, pref, off, nq, k, normalize, excl, false, xoff, nmax, rows, scores, out_count, max_rule);
    // host buffers: triggers and preferences in, rows and scores out, through the staging slot
    uint32_t* d_trig; double *d_pref, *d_sc; uint64_t* d_rows;
    if ((rc = scratch_carve(ctx, kSlotStaging, [&](Carve& c) {
            d_trig = c.take<uint32_t>(total);
            d_pref = c.take<double>(total);
            d_rows = c.take<uint64_t>((size_t)nq * k);
            d_sc = c.take<double>((size_t)nq * k);
        }))) return rc;
    uint32_t h_off[kMaxQueries + 1];
    for (uint32_t q = 0; q <= nq; ++q) h_off[q] = off[q] - off[0];
    if (total) {
        PG_HIP(hipMemcpyAsync(d_trig, trig + off[0], (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(d_pref, pref + off[0], (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = cf_recall_locked(who, ctx, s, d_trig, d_pref, h_off, nq, k, normalize, excl, true, xoff, nmax, d_rows, d_sc, out_count, max_rule);
    if (rc) return rc;
    PG_HIP(hipMemcpyAsync(rows, d_rows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(scores, d_sc, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

// RealTimeU2IRecall in one call: the trigger kernel writes each request's trigger list into kSlotRtU2I, the
// expansion kernel reads it through CfTrigDev; the two launches follow each other on the stream.  host: events in, answer out
// through the staging slot.
int rt_recall_entry(const char* who, pg_ctx* ctx, pg_rtu2i* c, const pg_simtable* s, const uint32_t* ev_rows, const uint16_t* ev_code,
                    const double* ev_pt, const int64_t* ev_time, const uint32_t* ev_off, const int64_t* now, uint32_t nq, uint32_t k,
                    const pg_cf_opts* opts, uint64_t* rows, double* scores, uint32_t* out_count, bool host) {
    int rc;
    uint32_t nmax = 0;
    PG_REQUIRE(ctx && c && s, "%s: NULL argument", who);
    if ((rc = rt_check(who, c, s->rows, ev_rows, ev_code, ev_time, ev_off, now, nq))) return rc;
    if ((rc = cf_check(who, ctx, s, nullptr, nullptr, nullptr, nq, k, opts, rows, scores, &nmax, true))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    TableRead tr(s->t->rw);
    std::shared_lock<std::shared_mutex> sr(s->rw);
    const uint64_t gen = s->t->generation.load(std::memory_order_relaxed);
    PG_REQUIRE(gen == s->gen, "%s: the similarity table describes generation %llu of its item table, which is at generation %llu (stale)",
               who, (unsigned long long)s->gen, (unsigned long long)gen);
    const uint64_t* excl = opts ? opts->excl_rows : nullptr;
    const uint32_t* xoff = opts ? opts->excl_offsets : nullptr;
    const uint32_t total = ev_off[nq] - ev_off[0];
    uint32_t h_off[kMaxQueries + 1];
    for (uint32_t q = 0; q <= nq; ++q) h_off[q] = host ? ev_off[q] - ev_off[0] : ev_off[q];
    uint32_t* d_er = nullptr; uint16_t* d_ec = nullptr; double *d_ep = nullptr, *d_sc = nullptr; int64_t* d_et = nullptr; uint64_t* d_rows = nullptr;
    if (host) {
        if ((rc = scratch_carve(ctx, kSlotStaging, [&](Carve& cv) {
                d_er = cv.take<uint32_t>(total);
                d_ec = cv.take<uint16_t>(total);
                d_ep = cv.take<double>(ev_pt ? total : 0);
                d_et = cv.take<int64_t>(total);
                d_rows = cv.take<uint64_t>((size_t)nq * k);
                d_sc = cv.take<double>((size_t)nq * k);
            }))) return rc;
        if (total) {
            PG_HIP(hipMemcpyAsync(d_er, ev_rows + ev_off[0], (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
            PG_HIP(hipMemcpyAsync(d_ec, ev_code + ev_off[0], (size_t)total * 2, hipMemcpyHostToDevice, ctx->stream));
            if (ev_pt) PG_HIP(hipMemcpyAsync(d_ep, ev_pt + ev_off[0], (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
            PG_HIP(hipMemcpyAsync(d_et, ev_time + ev_off[0], (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
        }
    }
    const auto make_trig = [&](CfTrigDev* td) {
        return rt_triggers_enqueue_locked(who, ctx, c, (uint32_t)s->rows, host ? d_er : ev_rows, host ? d_ec : ev_code,
                                          host ? (ev_pt ? d_ep : nullptr) : ev_pt, host ? d_et : ev_time, h_off, now, nq, nullptr, nullptr,
                                          nullptr, td);
    };
    rc = cf_recall_locked(who, ctx, s, nullptr, nullptr, nullptr, nq, k, 0, excl, host, xoff, nmax, host ? d_rows : rows, host ? d_sc : scores,
                          out_count, true, make_trig);
    if (rc || !host) return rc;
    PG_HIP(hipMemcpyAsync(rows, d_rows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(scores, d_sc, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_simtable_create(pg_ctx* ctx, const pg_table* t, pg_simtable** out) {
    PG_REQUIRE(ctx && t && out, "pg_simtable_create: NULL argument");
    PG_REQUIRE(t->rows >= 1 && t->rows <= 0xFFFFFFFFull, "pg_simtable_create: a table of %llu rows (1 .. 2^32 - 1)", (unsigned long long)t->rows);
    PG_REQUIRE(!t->d_row_map, "pg_simtable_create: a filtered view has no similarity table (its rows are not the source's)");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    pg::TableRead tr(t->rw);
    pg_simtable* s = new pg_simtable();
    s->t = t;
    s->gen = t->generation.load(std::memory_order_relaxed);
    s->rows = t->rows;
    const hipError_t e = hipMalloc((void**)&s->d_off, (s->rows + 1) * 8);
    if (e != hipSuccess) {
        pg::set_error("pg_simtable_create: hipMalloc(%.1f MB) failed: %s", (double)((s->rows + 1) * 8) / 1e6, hipGetErrorString(e));
        delete s;
        return PG_ERR_NOMEM;
    }
    // a table whose rows were never uploaded has empty lists
    if (hipMemsetAsync(s->d_off, 0, (s->rows + 1) * 8, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        pg::set_error("pg_simtable_create: clearing the offsets failed");
        (void)hipFree(s->d_off);
        delete s;
        return PG_ERR_DEVICE;
    }
    *out = s;
    return PG_OK;
}

int pg_simtable_upload(pg_ctx* ctx, pg_simtable* s, uint64_t row0, uint64_t nrows, const uint64_t* offsets, const uint32_t* nbr_rows,
                       const float* sims) {
    PG_REQUIRE(ctx && s && offsets, "pg_simtable_upload: NULL argument");
    PG_REQUIRE(row0 <= s->rows && nrows <= s->rows - row0, "pg_simtable_upload: rows [%llu, %llu) outside the table's %llu",
               (unsigned long long)row0, (unsigned long long)(row0 + nrows), (unsigned long long)s->rows);
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> sw(s->rw);
    PG_REQUIRE(row0 >= s->rows_uploaded, "pg_simtable_upload: row %llu after rows up to %llu were uploaded (rows arrive in ascending order)",
               (unsigned long long)row0, (unsigned long long)s->rows_uploaded);
    const uint64_t total = offsets[nrows] - offsets[0];
    PG_REQUIRE(offsets[nrows] >= offsets[0] && (total == 0 || (nbr_rows && sims)), "pg_simtable_upload: NULL argument");
    // every refusal comes before the first change: a refused upload leaves the table as it was
    std::vector<uint32_t> seen;
    for (uint64_t r = 0; r < nrows; ++r) {
        PG_REQUIRE(offsets[r + 1] >= offsets[r], "pg_simtable_upload: offsets[%llu] is below offsets[%llu]", (unsigned long long)(r + 1),
                   (unsigned long long)r);
        const uint64_t b = offsets[r], len = offsets[r + 1] - b;
        PG_REQUIRE(len <= pg::kCfMaxList, "pg_simtable_upload: the list of row %llu has %llu entries (at most %u)", (unsigned long long)(row0 + r),
                   (unsigned long long)len, pg::kCfMaxList);
        for (uint64_t i = 0; i < len; ++i) {
            PG_REQUIRE(nbr_rows[b + i] < s->rows, "pg_simtable_upload: neighbour %u of row %llu is outside the table's %llu rows", nbr_rows[b + i],
                       (unsigned long long)(row0 + r), (unsigned long long)s->rows);
            PG_REQUIRE(std::isfinite(sims[b + i]), "pg_simtable_upload: a similarity of row %llu is not finite", (unsigned long long)(row0 + r));
        }
        seen.assign(nbr_rows + b, nbr_rows + b + len);
        std::sort(seen.begin(), seen.end());
        for (uint64_t i = 1; i < len; ++i)
            PG_REQUIRE(seen[i] != seen[i - 1], "pg_simtable_upload: neighbour %u appears twice in the list of row %llu", seen[i],
                       (unsigned long long)(row0 + r));
    }
    if (nrows == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    if (s->pairs + total > s->cap) {
        const uint64_t cap = std::max<uint64_t>(s->pairs + total, s->cap + s->cap / 2);
        uint32_t* nn = nullptr;
        float* ns = nullptr;
        if (hipMalloc((void**)&nn, cap * 4) != hipSuccess || hipMalloc((void**)&ns, cap * 4) != hipSuccess) {
            if (nn) (void)hipFree(nn);
            pg::set_error("pg_simtable_upload: hipMalloc(%.1f MB) failed", (double)(cap * 8) / 1e6);
            return PG_ERR_NOMEM;
        }
        PG_HIP(hipDeviceSynchronize());                  // (no other context's recall still reads the old arrays: they hold the shared lock until they are synchronised)
        if (s->pairs) {
            PG_HIP(hipMemcpyAsync(nn, s->d_nbr, s->pairs * 4, hipMemcpyDeviceToDevice, ctx->stream));
            PG_HIP(hipMemcpyAsync(ns, s->d_sim, s->pairs * 4, hipMemcpyDeviceToDevice, ctx->stream));
            PG_HIP(hipStreamSynchronize(ctx->stream));
        }
        if (s->d_nbr) (void)hipFree(s->d_nbr);
        if (s->d_sim) (void)hipFree(s->d_sim);
        s->d_nbr = nn;
        s->d_sim = ns;
        s->cap = cap;
    }
    std::vector<uint64_t> abs(nrows);
    for (uint64_t r = 0; r < nrows; ++r) abs[r] = s->pairs + (offsets[r] - offsets[0]);
    PG_HIP(hipMemcpyAsync(s->d_off + row0, abs.data(), nrows * 8, hipMemcpyHostToDevice, ctx->stream));
    // (the rows between the last upload and row0 already end at the old total: their lists stay empty)
    const uint64_t tail = s->rows + 1 - (row0 + nrows);
    pg::cf_fill_u64_kernel<<<(unsigned)std::min<uint64_t>((tail + 255) / 256, 4096), 256, 0, ctx->stream>>>(s->d_off + row0 + nrows, tail,
                                                                                                          s->pairs + total);
    PG_HIP(hipGetLastError());
    if (total) {
        PG_HIP(hipMemcpyAsync(s->d_nbr + s->pairs, nbr_rows + offsets[0], total * 4, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(s->d_sim + s->pairs, sims + offsets[0], total * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    PG_HIP(hipStreamSynchronize(ctx->stream));
    s->pairs += total;
    s->rows_uploaded = row0 + nrows;
    return PG_OK;
}

int pg_simtable_info(const pg_simtable* s, uint64_t* rows, uint64_t* pairs, uint64_t* rows_uploaded, uint64_t* generation) {
    PG_REQUIRE(s, "pg_simtable_info: table is NULL");
    std::shared_lock<std::shared_mutex> sr(s->rw);
    if (rows) *rows = s->rows;
    if (pairs) *pairs = s->pairs;
    if (rows_uploaded) *rows_uploaded = s->rows_uploaded;
    if (generation) *generation = s->gen;
    return PG_OK;
}

int pg_simtable_destroy(pg_ctx* ctx, pg_simtable* s) {
    PG_REQUIRE(ctx, "pg_simtable_destroy: ctx is NULL");
    if (!s) return PG_OK;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        std::unique_lock<std::shared_mutex> sw(s->rw);
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipDeviceSynchronize());
        if (s->d_off) (void)hipFree(s->d_off);
        if (s->d_nbr) (void)hipFree(s->d_nbr);
        if (s->d_sim) (void)hipFree(s->d_sim);
    }
    delete s;
    return PG_OK;
}

int pg_cf_recall(pg_ctx* ctx, const pg_simtable* s, const uint32_t* trigger_rows, const double* trigger_prefer, const uint32_t* trigger_offsets,
                 uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count) {
    return pg::cf_entry("pg_cf_recall", ctx, s, trigger_rows, trigger_prefer, trigger_offsets, nq, k, opts, out_rows, out_scores, out_count, true);
}

int pg_cf_recall_dev(pg_ctx* ctx, const pg_simtable* s, const uint32_t* d_trigger_rows, const double* d_trigger_prefer,
                     const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* d_out_rows,
                     double* d_out_scores, uint32_t* out_count) {
    return pg::cf_entry("pg_cf_recall_dev", ctx, s, d_trigger_rows, d_trigger_prefer, trigger_offsets, nq, k, opts, d_out_rows, d_out_scores,
                        out_count, false);
}

int pg_rtu2i_expand(pg_ctx* ctx, const pg_simtable* s, const uint32_t* trigger_rows, const double* trigger_prefer, const uint32_t* trigger_offsets,
                    uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count) {
    return pg::cf_entry("pg_rtu2i_expand", ctx, s, trigger_rows, trigger_prefer, trigger_offsets, nq, k, opts, out_rows, out_scores, out_count, true,
                        true);
}

int pg_rtu2i_expand_dev(pg_ctx* ctx, const pg_simtable* s, const uint32_t* d_trigger_rows, const double* d_trigger_prefer,
                        const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* d_out_rows,
                        double* d_out_scores, uint32_t* out_count) {
    return pg::cf_entry("pg_rtu2i_expand_dev", ctx, s, d_trigger_rows, d_trigger_prefer, trigger_offsets, nq, k, opts, d_out_rows, d_out_scores,
                        out_count, false, true);
}

int pg_rtu2i_recall(pg_ctx* ctx, pg_rtu2i* c, const pg_simtable* s, const uint32_t* event_rows, const uint16_t* event_code,
                    const double* event_play_time, const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now, uint32_t nq,
                    uint32_t k, const pg_cf_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count) {
    return pg::rt_recall_entry("pg_rtu2i_recall", ctx, c, s, event_rows, event_code, event_play_time, event_time, event_offsets, now, nq, k, opts,
                               out_rows, out_scores, out_count, true);
}

int pg_rtu2i_recall_dev(pg_ctx* ctx, pg_rtu2i* c, const pg_simtable* s, const uint32_t* d_event_rows, const uint16_t* d_event_code,
                        const double* d_event_play_time, const int64_t* d_event_time, const uint32_t* event_offsets, const int64_t* now,
                        uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* d_out_rows, double* d_out_scores, uint32_t* out_count) {
    return pg::rt_recall_entry("pg_rtu2i_recall_dev", ctx, c, s, d_event_rows, d_event_code, d_event_play_time, d_event_time, event_offsets, now, nq,
                               k, opts, d_out_rows, d_out_scores, out_count, false);
}

}  // extern "C"
