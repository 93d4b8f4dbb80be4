// x2i.hip — U2I2X2I recall over an HBM X table: trigger items -> their X values (category, author, tags) -> the
// items listed under each X.
//
// UserCollaborativeFilterRecall and RealTimeU2IRecall switch to this two-hop form when a config names Item2XTable and X2ItemTable
// (module/user_collaborative_dao.go:24-26).  Both DAOs (module/user_collaborative_u2i2x2i_hologres_dao.go:73-348,
// module/realtime_user2item_u2i2x2i_hologres_dao.go:94-270) add a trigger's preference to every X of the trigger
// (xPreferScoreMap[x] += prefer, :196-211 / :161-175), walk the "id:score,..." row of every distinct X, skip the ids that are
// trigger items (:311-315 / :242-246) and give every other entry the score xPrefer[x] * score.  The collaborative DAO sums an
// item's entries in float64 and divides by the largest sum unless Normalization is "off"
// (mergeUserCollaborativeItemsResult, user_collaborative_dao.go:38-68); the realtime DAO keeps an item's largest entry
// (a descending sort, then uniqItems, :262-263).
//
// Storage: two CSR structures over the local rows of an item table and n_x dictionary codes — item -> X (offsets uint64
// [rows + 1], x ids uint32) and X -> items (offsets uint64[n_x + 1], item rows uint32, scores float, widened exactly when used).
//
// One workgroup of 1024 lanes serves one request in one launch.  Hop 1 is a keyed fp64 reduction over X in an open-addressed
// LDS table that lies in the bytes hop 2's table takes afterwards: one trigger per step with a barrier between steps, the
// trigger's X list (at most 64 entries, duplicate-free) over the lanes of the first wave, the slot's key claimed by
// compare-and-swap and the preference added with a plain read-modify-write — the determinism argument of cf.hip, no
// floating-point atomics.  A new X takes its first-appearance rank from the running count plus its ballot rank.  The X are then
// staged in that order as (list begin, length, xPrefer), the non-finite sums dropped, and hop 2 IS cf.hip's accumulation
// (cf_kernel.hpp: cf_accumulate with the staged X as its triggers) with one test in front of the slot claim: an item that is
// one of the request's trigger rows, looked up in a small LDS set, is dropped.  The maximum, the normalisation, the sort, the
// cut and the padding are cf_finish, unchanged.
#include "cf_kernel.hpp"
#include "x2i_host.hpp"

#include <cmath>
#include <functional>

struct pg_xtable {
    // recalls share this lock, the uploads take it exclusively.  Lock order: ctx->mu, the item table, then this.
    mutable std::shared_mutex rw;
    const pg_table* t = nullptr;
    uint64_t gen = 0;              // t->generation at create: a recall on another generation is refused
    uint64_t rows = 0;
    uint32_t n_x = 0;
    // one CSR side: offsets [n + 1], ids [cap] with `pairs` used, scores beside them (the X -> items side only)
    struct Side {
        uint64_t n = 0;
        uint64_t* d_off = nullptr;
        uint32_t* d_id = nullptr;
        float* d_sc = nullptr;
        uint64_t pairs = 0, cap = 0;
        uint64_t uploaded = 0;     // the next upload starts at or behind this key
    } i2x, x2i;
};

namespace pg {
namespace {

// LDS.  Hop 2's table: 10240 slots of (fp64 accumulator, uint32 key) in two planes = 120 KiB, load factor <= 0.5: the LDS tier
// serves requests of at most 5120 (X, item) pairs (cf.hip's table has 12288 slots; the 24 KiB difference holds the staged X).
// Hop 1's table lies in the same bytes: 4096 slots of (fp64 sum, uint32 key) = 48 KiB and the occupied slots by rank behind
// them; it never holds more than kX2iMaxX + kX2iMaxXPerItem keys (a request beyond kX2iMaxX stops inserting).  The sort orders
// kCfSortChunk records = 128 KiB from the start of the LDS: the table and the head of the staged X, both dead by then.
constexpr uint32_t kX2iLdsSlots = 10240;
constexpr uint32_t kX2iLdsMaxPairs = kX2iLdsSlots / 2;
constexpr size_t kX2iTableBytes = (size_t)kX2iLdsSlots * 12;
constexpr uint32_t kX2iXSlots = 4096;
constexpr uint32_t kX2iXCap = kX2iMaxX + kX2iMaxXPerItem;        // the most keys hop 1's table and rank list ever hold
constexpr uint32_t kX2iTrigSlots = 512;                         // the trigger set: <= 256 keys
static_assert(kX2iLdsSlots % kCfThreads == 0, "cf_accumulate walks the table in strides of the workgroup");
static_assert((size_t)kX2iXSlots * 12 + (size_t)kX2iXCap * 4 <= kX2iTableBytes, "hop 1's table lies in hop 2's bytes");
static_assert(kX2iXCap * 2 <= kX2iXSlots, "hop 1's load factor");
static_assert(kX2iMaxX == kCfThreads && kX2iMaxList <= kCfThreads && kX2iMaxPairs == kCfMaxPairs && kX2iMaxTriggers == kCfMaxTriggers &&
                  kX2iMaxK == kCfMaxDepth && kX2iMaxExclude == kMaxExclude && kX2iMaxQueries == (uint32_t)kMaxQueries,
              "the host statement's limits are the kernel's");
constexpr size_t kX2iStageAt = kX2iTableBytes;                                   // st_begin u64, st_pref f64, st_len u32 [kX2iMaxX]
constexpr size_t kX2iTrigAt = kX2iStageAt + (size_t)kX2iMaxX * (8 + 8 + 4);      // tg_begin u64, tg_pref f64, tg_len u32 [256]
constexpr size_t kX2iSetAt = kX2iTrigAt + (size_t)kCfMaxTriggers * (8 + 8 + 4);
constexpr size_t kX2iWordsAt = kX2iSetAt + (size_t)kX2iTrigSlots * 4;            // scan sums [16], max_bits, n_pairs, n_items, n_x
constexpr size_t kX2iLds = kX2iWordsAt + 16 * 4 + 8 + 3 * 4 + 4;
static_assert((size_t)kCfSortChunk * 16 <= kX2iWordsAt, "the sort's LDS ends in front of the words cf_finish reads");
static_assert(kX2iLds <= 160 * 1024, "one workgroup's LDS");

struct X2iArgs {
    CfArgs cf;                     // off / nbr / sim: the X -> items side; rows, triggers, tiers and outputs as in cf.hip
    const uint64_t* i2x_off;       // [rows + 1]
    const uint32_t* i2x_ids;
    uint32_t n_x;
};

// is `item` one of the request's trigger rows?
struct X2iSkip {
    const uint32_t* set;
    __device__ __forceinline__ bool operator()(uint32_t item) const {
        for (uint32_t h = cf_slot(item, kX2iTrigSlots);; h = (h + 1) & (kX2iTrigSlots - 1)) {
            const uint32_t c = set[h];
            if (c == item) return true;
            if (c == kCfEmpty) return false;
        }
    }
};

// Request q = blockIdx.x.  trigger_prefer must be finite (the host-array entry points check it).
template <bool kMax>
__global__ __launch_bounds__(kCfThreads) void x2i_recall_kernel(X2iArgs xa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char x2i_lds[];
    const CfArgs& a = xa.cf;
    uint64_t* st_begin = reinterpret_cast<uint64_t*>(x2i_lds + kX2iStageAt);
    double* st_pref = reinterpret_cast<double*>(st_begin + kX2iMaxX);
    uint32_t* st_len = reinterpret_cast<uint32_t*>(st_pref + kX2iMaxX);
    uint64_t* tg_begin = reinterpret_cast<uint64_t*>(x2i_lds + kX2iTrigAt);
    double* tg_pref = reinterpret_cast<double*>(tg_begin + kCfMaxTriggers);
    uint32_t* tg_len = reinterpret_cast<uint32_t*>(tg_pref + kCfMaxTriggers);
    uint32_t* tset = reinterpret_cast<uint32_t*>(x2i_lds + kX2iSetAt);
    uint32_t* ws = reinterpret_cast<uint32_t*>(x2i_lds + kX2iWordsAt);
    unsigned long long* max_bits = reinterpret_cast<unsigned long long*>(ws + 16);
    uint32_t* n_pairs = reinterpret_cast<uint32_t*>(max_bits + 1);
    uint32_t* n_items = n_pairs + 1;
    uint32_t* n_x = n_items + 1;
    // hop 1's table, in the bytes of hop 2's
    double* xacc = reinterpret_cast<double*>(x2i_lds);
    uint32_t* xkeys = reinterpret_cast<uint32_t*>(xacc + kX2iXSlots);
    uint32_t* xlist = xkeys + kX2iXSlots;            // [kX2iXCap] the occupied slots in order of first appearance
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t t0 = a.trig_off ? a.trig_off[q] : q * a.trig_stride;
    const uint32_t nt = min(a.trig_off ? a.trig_off[q + 1] - t0 : min(a.trig_cnt[q], a.trig_stride), kCfMaxTriggers);
    if (tid == 0) {
        *max_bits = 0;
        *n_pairs = 0;
        *n_items = 0;
        *n_x = 0;
    }
    for (uint32_t i = tid; i < kX2iTrigSlots; i += kCfThreads) tset[i] = kCfEmpty;
    for (uint32_t i = tid; i < kX2iXSlots; i += kCfThreads) xkeys[i] = kCfEmpty;
    __syncthreads();
    // ---- stage the triggers, build the set of their rows ----
    if (tid < nt) {
        // a trigger of UINT32_MAX or >= rows contributes nothing: the id the reference's SQL does not return
        const uint32_t r = a.trig[t0 + tid];
        uint64_t b = 0;
        uint32_t len = 0;
        if (r < a.rows) {
            b = xa.i2x_off[r];
            len = min((uint32_t)(xa.i2x_off[r + 1] - b), kX2iMaxXPerItem);
            for (uint32_t h = cf_slot(r, kX2iTrigSlots);; h = (h + 1) & (kX2iTrigSlots - 1)) {
                const uint32_t cur = atomicCAS(&tset[h], kCfEmpty, r);
                if (cur == kCfEmpty || cur == r) break;
            }
        }
        tg_begin[tid] = b;
        tg_len[tid] = len;
        tg_pref[tid] = a.pref[t0 + tid];
    }
    __syncthreads();
    // ---- hop 1: one trigger per step, its X list over the lanes of wave 0 ----
    uint32_t x_next = kCfEmpty;
    if (nt && tid < tg_len[0]) x_next = xa.i2x_ids[tg_begin[0] + tid];
    for (uint32_t j = 0; j < nt; ++j) {
        if (tid < (uint32_t)kWave) {
            const uint32_t x = x_next;
            const uint32_t len = tg_len[j];
            const double pf = tg_pref[j];
            x_next = kCfEmpty;
            if (j + 1 < nt && tid < tg_len[j + 1]) x_next = xa.i2x_ids[tg_begin[j + 1] + tid];
            const uint32_t cnt = *n_x;                   // (only this wave writes it, in program order behind this read)
            bool fresh = false;
            uint32_t mine_at = 0;
            // a request already beyond kX2iMaxX is reported: it stops inserting, so the table never overflows
            if (tid < len && x < xa.n_x && cnt <= kX2iMaxX) {
                for (uint32_t h = cf_slot(x, kX2iXSlots);; h = (h + 1) & (kX2iXSlots - 1)) {
                    uint32_t cur = __hip_atomic_load(&xkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    bool mine = false;
                    if (cur == kCfEmpty) {
                        cur = atomicCAS(&xkeys[h], kCfEmpty, x);
                        mine = cur == kCfEmpty;
                    }
                    if (mine) {
                        xacc[h] = pf;                    // the first trigger that names an X sets its preference
                        fresh = true;
                        mine_at = h;
                        break;
                    }
                    if (cur == x) {
                        xacc[h] = xacc[h] + pf;
                        break;
                    }
                }
            }
            // first-appearance rank: the running count plus the new X in the lanes (= list positions) before this one
            const unsigned long long m = __ballot(fresh);
            if (fresh) xlist[cnt + ballot_rank(m)] = mine_at;
            if (tid == 0 && m) *n_x = cnt + (uint32_t)__popcll(m);
        }
        __syncthreads();                                 // trigger j's additions are done, and visible, before trigger j + 1's
    }
    const uint32_t nx = *n_x;
    if (nx > kX2iMaxX) {
        if (tid == 0) {
            atomicMin(a.status, q * 2u);
            a.out_count[q] = 0;
        }
        cf_pad(a, q, 0);
        return;
    }
    // ---- stage the X in rank order, the non-finite sums dropped (lane r = rank r: kX2iMaxX == kCfThreads) ----
    uint32_t x = 0;
    double pf = 0.0;
    bool keep = false;
    if (tid < nx) {
        const uint32_t h = xlist[tid];
        x = xkeys[h];
        pf = xacc[h];
        keep = isfinite(pf);
    }
    uint32_t nkept;
    const uint32_t pos = block_excl_scan<kCfThreads / kWave, uint32_t>(keep ? 1u : 0u, ws, &nkept);
    if (keep) {
        const uint64_t b = a.off[x];
        const uint32_t len = min((uint32_t)(a.off[x + 1] - b), kX2iMaxList);
        st_begin[pos] = b;
        st_len[pos] = len;
        st_pref[pos] = pf;
        if (len) atomicAdd(n_pairs, len);
    }
    __syncthreads();                                     // hop 1's table is dead from here: cf_accumulate clears its own
    const uint32_t pairs = *n_pairs;
    if (pairs > kCfMaxPairs) {
        if (tid == 0) {
            atomicMin(a.status, q * 2u + 1u);
            a.out_count[q] = 0;
        }
        cf_pad(a, q, 0);
        return;
    }
    // ---- hop 2: cf.hip's accumulation with the staged X as its triggers ----
    ulonglong2* cand = a.cand + (size_t)q * a.cand_cap;
    const X2iSkip skip{tset};
    if (pairs <= min(a.lds_max_pairs, kX2iLdsMaxPairs)) {
        double* acc = reinterpret_cast<double*>(x2i_lds);
        uint32_t* keys = reinterpret_cast<uint32_t*>(x2i_lds + (size_t)kX2iLdsSlots * 8);
        cf_accumulate<true, kMax>(a, keys, acc, kX2iLdsSlots, nkept, st_begin, st_pref, st_len, cand, n_items, max_bits, skip);
    } else {
        uint32_t slots = kCfThreads;
        while (slots < 2 * pairs) slots <<= 1;
        slots = min(slots, a.gslots);                    // (distinct items <= min(pairs, rows) <= gslots / 2 either way)
        cf_accumulate<false, kMax>(a, a.gkeys + (size_t)q * a.gslots, a.gacc + (size_t)q * a.gslots, slots, nkept, st_begin, st_pref, st_len,
                                   cand, n_items, max_bits, skip);
    }
    cf_finish(a, q, cand, n_items, max_bits, x2i_lds);
}

int x2i_fail(int rc, const std::string& err) {
    set_error("%s", err.c_str());
    return rc;
}

int x2i_stale_check(const char* who, const pg_xtable* s) {
    const uint64_t gen = s->t->generation.load(std::memory_order_relaxed);
    PG_REQUIRE(gen == s->gen, "%s: the X table describes generation %llu of its item table, which is at generation %llu (stale)", who,
               (unsigned long long)s->gen, (unsigned long long)gen);
    return PG_OK;
}

// The recall of nq requests whose triggers are device memory (indexed by the host offsets `off` as given) into device outputs
// [nq][k]; lists: host ids (staged here) or device ids, host offsets.  Caller holds ctx->mu, the item table's shared lock and
// the X table's; ends synchronised.  With `off` NULL the triggers are what make_trig describes: it is called once everything
// of this call is staged and its staging synchronised, right in front of the launch (cf.hip's cf_recall_locked, whose scratch
// layout this follows in a slot of its own).  *reported: the call returns PG_ERR_UNSUPPORTED because a request is beyond a limit —
// every other request's outputs and counts are written.
int x2i_recall_locked(const char* who, pg_ctx* ctx, const pg_xtable* s, const uint32_t* d_trig, const double* d_pref, const uint32_t* off,
                      uint32_t nq, uint32_t k, int normalize, bool max_rule, const uint64_t* excl, bool excl_on_host, const uint32_t* xoff,
                      uint32_t nmax, uint64_t* d_out_rows, double* d_out_scores, uint32_t* out_count, bool* reported,
                      const std::function<int(CfTrigDev*)>& make_trig = nullptr) {
    int rc;
    *reported = false;
    const uint32_t rows_eff = (uint32_t)std::min<uint64_t>(kCfMaxPairs, s->rows);
    uint32_t gslots = kCfThreads, cand_cap = 1;
    while (gslots < 2 * rows_eff) gslots <<= 1;
    while (cand_cap < rows_eff) cand_cap <<= 1;
    const uint32_t kd = k + nmax;
    const uint32_t xtotal = nmax && excl_on_host ? xoff[nq] - xoff[0] : 0;
    uint32_t *d_status, *d_off, *d_xoff, *d_keys; uint64_t *d_list, *d_xrows; double *d_acc, *d_xsc; ulonglong2* d_cand; float *d_xidx, *d_oidx;
    if ((rc = scratch_carve(ctx, kSlotX2i, [&](Carve& c) {
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
    X2iArgs xa;
    CfArgs& a = xa.cf;
    xa.i2x_off = s->i2x.d_off;
    xa.i2x_ids = s->i2x.d_id;
    xa.n_x = s->n_x;
    a.off = s->x2i.d_off;
    a.nbr = s->x2i.d_id;
    a.sim = s->x2i.d_sc;
    a.rows = (uint32_t)s->rows;
    a.row_offset = s->t->row_offset;
    a.trig = off ? d_trig : td.d_rows;
    a.pref = off ? d_pref : td.d_weight;
    a.trig_off = off ? d_off : nullptr;
    a.trig_cnt = td.d_count;
    a.trig_stride = td.stride;
    a.lds_max_pairs = std::min(ctx->knobs.cf_lds_max_pairs, kX2iLdsMaxPairs);
    a.gslots = gslots;
    a.gkeys = d_keys;
    a.gacc = d_acc;
    a.cand = d_cand;
    a.cand_cap = cand_cap;
    a.normalize = max_rule ? 0 : normalize;
    a.kd = kd;
    a.out_rows = nmax ? d_xrows : d_out_rows;
    a.out_scores = nmax ? d_xsc : d_out_scores;
    a.out_idx = nmax ? d_xidx : nullptr;
    a.out_count = d_status + 1;
    a.status = d_status;
    if (max_rule) {
        if ((rc = ensure_dyn_lds(ctx, (const void*)x2i_recall_kernel<true>, kX2iLds))) return rc;
        x2i_recall_kernel<true><<<nq, kCfThreads, kX2iLds, ctx->stream>>>(xa);
    } else {
        if ((rc = ensure_dyn_lds(ctx, (const void*)x2i_recall_kernel<false>, kX2iLds))) return rc;
        x2i_recall_kernel<false><<<nq, kCfThreads, kX2iLds, ctx->stream>>>(xa);
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
    if (out_count) memcpy(out_count, ctx->h_status + 1, (size_t)nq * 4);
    if (ctx->h_status[0] != kX2iNone) {
        *reported = true;
        return x2i_fail(PG_ERR_UNSUPPORTED, x2i_limit_message(who, ctx->h_status[0]));
    }
    return PG_OK;
}

int x2i_entry(const char* who, pg_ctx* ctx, const pg_xtable* s, const uint32_t* trig, const double* pref, const uint32_t* off, uint32_t nq,
              uint32_t k, const pg_x2i_opts* opts, uint64_t* rows, double* scores, uint32_t* out_count, bool host) {
    int rc;
    uint32_t nmax = 0;
    std::string err;
    PG_REQUIRE(ctx && s, "%s: NULL argument", who);
    if ((rc = x2i_check_args(who, trig, pref, off, nq, k, opts, rows, scores, false, host, &nmax, &err))) return x2i_fail(rc, err);
    const uint32_t total = off[nq] - off[0];
    const bool max_rule = opts && opts->max_rule;
    const int normalize = opts ? opts->normalize : 1;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    TableRead tr(s->t->rw);
    std::shared_lock<std::shared_mutex> sr(s->rw);
    if ((rc = x2i_stale_check(who, s))) return rc;
    const uint64_t* excl = opts ? opts->excl_rows : nullptr;
    const uint32_t* xoff = opts ? opts->excl_offsets : nullptr;
    bool reported;
    if (!host)
        return x2i_recall_locked(who, ctx, s, trig, pref, off, nq, k, normalize, max_rule, excl, false, xoff, nmax, rows, scores, out_count,
                                 &reported);
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
    rc = x2i_recall_locked(who, ctx, s, d_trig, d_pref, h_off, nq, k, normalize, max_rule, excl, true, xoff, nmax, d_rows, d_sc, out_count,
                           &reported);
    // (a request beyond a limit is reported, the other requests' outputs are written all the same)
    if (rc && !reported) return rc;
    PG_HIP(hipMemcpyAsync(rows, d_rows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(scores, d_sc, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return rc;
}

// RealTimeU2IRecall over an X table in one call: the trigger kernel writes each request's trigger list into kSlotRtU2I, the
// x2i kernel reads it through CfTrigDev; the two launches follow each other on the stream.  host: events in, answer out through
// the staging slot.
int rt_x_recall_entry(const char* who, pg_ctx* ctx, pg_rtu2i* c, const pg_xtable* s, const uint32_t* ev_rows, const uint16_t* ev_code,
                      const double* ev_pt, const int64_t* ev_time, const uint32_t* ev_off, const int64_t* now, uint32_t nq, uint32_t k,
                      const pg_x2i_opts* opts, uint64_t* rows, double* scores, uint32_t* out_count, bool host) {
    int rc;
    uint32_t nmax = 0;
    std::string err;
    PG_REQUIRE(ctx && c && s, "%s: NULL argument", who);
    if ((rc = rt_check(who, c, s->rows, ev_rows, ev_code, ev_time, ev_off, now, nq))) return rc;
    if ((rc = x2i_check_args(who, nullptr, nullptr, nullptr, nq, k, opts, rows, scores, true, false, &nmax, &err))) return x2i_fail(rc, err);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    TableRead tr(s->t->rw);
    std::shared_lock<std::shared_mutex> sr(s->rw);
    if ((rc = x2i_stale_check(who, s))) return rc;
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
    bool reported;
    rc = x2i_recall_locked(who, ctx, s, nullptr, nullptr, nullptr, nq, k, 0, true, excl, host, xoff, nmax, host ? d_rows : rows,
                           host ? d_sc : scores, out_count, &reported, make_trig);
    if (!host || (rc && !reported)) return rc;
    PG_HIP(hipMemcpyAsync(rows, d_rows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(scores, d_sc, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return rc;
}

// One side's upload, validated by the caller: the lists of `count` keys from `first` appended behind the side's pairs.  Caller
// holds ctx->mu and the table's exclusive lock.
int x2i_side_append(const char* who, pg_ctx* ctx, pg_xtable::Side* sd, uint64_t first, uint64_t count, const uint64_t* offsets,
                    const uint32_t* ids, const float* scores) {
    if (count == 0) return PG_OK;
    const uint64_t total = offsets[count] - offsets[0];
    PG_HIP(hipSetDevice(ctx->device));
    if (sd->pairs + total > sd->cap) {
        const uint64_t cap = std::max<uint64_t>(sd->pairs + total, sd->cap + sd->cap / 2);
        uint32_t* ni = nullptr;
        float* ns = nullptr;
        if (hipMalloc((void**)&ni, cap * 4) != hipSuccess || (scores && hipMalloc((void**)&ns, cap * 4) != hipSuccess)) {
            if (ni) (void)hipFree(ni);
            set_error("%s: hipMalloc(%.1f MB) failed", who, (double)(cap * 8) / 1e6);
            return PG_ERR_NOMEM;
        }
        PG_HIP(hipDeviceSynchronize());                  // (no other context's recall still reads the old arrays: they hold the shared lock until they are synchronised)
        if (sd->pairs) {
            PG_HIP(hipMemcpyAsync(ni, sd->d_id, sd->pairs * 4, hipMemcpyDeviceToDevice, ctx->stream));
            if (scores) PG_HIP(hipMemcpyAsync(ns, sd->d_sc, sd->pairs * 4, hipMemcpyDeviceToDevice, ctx->stream));
            PG_HIP(hipStreamSynchronize(ctx->stream));
        }
        if (sd->d_id) (void)hipFree(sd->d_id);
        if (sd->d_sc) (void)hipFree(sd->d_sc);
        sd->d_id = ni;
        sd->d_sc = ns;
        sd->cap = cap;
    }
    std::vector<uint64_t> abs(count);
    for (uint64_t r = 0; r < count; ++r) abs[r] = sd->pairs + (offsets[r] - offsets[0]);
    PG_HIP(hipMemcpyAsync(sd->d_off + first, abs.data(), count * 8, hipMemcpyHostToDevice, ctx->stream));
    // (the keys between the last upload and `first` already end at the old total: their lists stay empty)
    const uint64_t tail = sd->n + 1 - (first + count);
    cf_fill_u64_kernel<<<(unsigned)std::min<uint64_t>((tail + 255) / 256, 4096), 256, 0, ctx->stream>>>(sd->d_off + first + count, tail,
                                                                                                      sd->pairs + total);
    PG_HIP(hipGetLastError());
    if (total) {
        PG_HIP(hipMemcpyAsync(sd->d_id + sd->pairs, ids + offsets[0], total * 4, hipMemcpyHostToDevice, ctx->stream));
        if (scores) PG_HIP(hipMemcpyAsync(sd->d_sc + sd->pairs, scores + offsets[0], total * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    PG_HIP(hipStreamSynchronize(ctx->stream));
    sd->pairs += total;
    sd->uploaded = first + count;
    return PG_OK;
}

void x2i_free_sides(pg_xtable* s) {
    for (pg_xtable::Side* sd : {&s->i2x, &s->x2i}) {
        if (sd->d_off) (void)hipFree(sd->d_off);
        if (sd->d_id) (void)hipFree(sd->d_id);
        if (sd->d_sc) (void)hipFree(sd->d_sc);
    }
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_xtable_create(pg_ctx* ctx, const pg_table* t, uint32_t n_x, pg_xtable** out) {
    PG_REQUIRE(ctx && t && out, "pg_xtable_create: NULL argument");
    PG_REQUIRE(t->rows >= 1 && t->rows < 0xFFFFFFFFull, "pg_xtable_create: a table of %llu rows (1 .. 2^32 - 2)", (unsigned long long)t->rows);
    PG_REQUIRE(n_x >= 1 && n_x < 0xFFFFFFFFu, "pg_xtable_create: n_x=%u (1 .. 2^32 - 2)", n_x);
    PG_REQUIRE(!t->d_row_map, "pg_xtable_create: a filtered view has no X table (its rows are not the source's)");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    pg::TableRead tr(t->rw);
    pg_xtable* s = new pg_xtable();
    s->t = t;
    s->gen = t->generation.load(std::memory_order_relaxed);
    s->rows = t->rows;
    s->n_x = n_x;
    s->i2x.n = s->rows;
    s->x2i.n = n_x;
    for (pg_xtable::Side* sd : {&s->i2x, &s->x2i}) {
        const hipError_t e = hipMalloc((void**)&sd->d_off, (sd->n + 1) * 8);
        if (e != hipSuccess) {
            sd->d_off = nullptr;
            pg::set_error("pg_xtable_create: hipMalloc(%.1f MB) failed: %s", (double)((sd->n + 1) * 8) / 1e6, hipGetErrorString(e));
            pg::x2i_free_sides(s);
            delete s;
            return PG_ERR_NOMEM;
        }
        // a side whose keys were never uploaded has empty lists
        if (hipMemsetAsync(sd->d_off, 0, (sd->n + 1) * 8, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            pg::set_error("pg_xtable_create: clearing the offsets failed");
            pg::x2i_free_sides(s);
            delete s;
            return PG_ERR_DEVICE;
        }
    }
    *out = s;
    return PG_OK;
}

int pg_xtable_upload_item2x(pg_ctx* ctx, pg_xtable* s, uint64_t row0, uint64_t nrows, const uint64_t* offsets, const uint32_t* x_ids) {
    const char* who = "pg_xtable_upload_item2x";
    PG_REQUIRE(ctx && s && offsets, "%s: NULL argument", who);
    PG_REQUIRE(row0 <= s->rows && nrows <= s->rows - row0, "%s: rows [%llu, %llu) outside the table's %llu", who, (unsigned long long)row0,
               (unsigned long long)(row0 + nrows), (unsigned long long)s->rows);
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> sw(s->rw);
    PG_REQUIRE(row0 >= s->i2x.uploaded, "%s: row %llu after rows up to %llu were uploaded (rows arrive in ascending order)", who,
               (unsigned long long)row0, (unsigned long long)s->i2x.uploaded);
    // every refusal comes before the first change: a refused upload leaves the table as it was
    std::string err;
    if (!pg::x2i_validate_lists(who, "row", "x id", row0, nrows, offsets, x_ids, nullptr, pg::kX2iMaxXPerItem, s->n_x, &err))
        return pg::x2i_fail(PG_ERR_INVALID, err);
    return pg::x2i_side_append(who, ctx, &s->i2x, row0, nrows, offsets, x_ids, nullptr);
}

int pg_xtable_upload_x2item(pg_ctx* ctx, pg_xtable* s, uint32_t x0, uint32_t nx, const uint64_t* offsets, const uint32_t* item_rows,
                            const float* scores) {
    const char* who = "pg_xtable_upload_x2item";
    PG_REQUIRE(ctx && s && offsets, "%s: NULL argument", who);
    PG_REQUIRE(x0 <= s->n_x && nx <= s->n_x - x0, "%s: X [%u, %llu) outside the table's %u", who, x0, (unsigned long long)x0 + nx, s->n_x);
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> sw(s->rw);
    PG_REQUIRE(x0 >= s->x2i.uploaded, "%s: X %u after X up to %llu were uploaded (X arrive in ascending order)", who, x0,
               (unsigned long long)s->x2i.uploaded);
    std::string err;
    bool any = false;
    for (uint32_t i = 0; i < nx && !any; ++i) any = offsets[i + 1] > offsets[i];
    PG_REQUIRE(!any || (item_rows && scores), "%s: NULL argument", who);
    if (!pg::x2i_validate_lists(who, "X", "item row", x0, nx, offsets, item_rows, scores, pg::kX2iMaxList, s->rows, &err))
        return pg::x2i_fail(PG_ERR_INVALID, err);
    return pg::x2i_side_append(who, ctx, &s->x2i, x0, nx, offsets, item_rows, scores);
}

int pg_xtable_info(const pg_xtable* s, uint64_t* rows, uint32_t* n_x, uint64_t* i2x_pairs, uint64_t* x2i_pairs, uint64_t* generation) {
    PG_REQUIRE(s, "pg_xtable_info: table is NULL");
    std::shared_lock<std::shared_mutex> sr(s->rw);
    if (rows) *rows = s->rows;
    if (n_x) *n_x = s->n_x;
    if (i2x_pairs) *i2x_pairs = s->i2x.pairs;
    if (x2i_pairs) *x2i_pairs = s->x2i.pairs;
    if (generation) *generation = s->gen;
    return PG_OK;
}

int pg_xtable_destroy(pg_ctx* ctx, pg_xtable* s) {
    PG_REQUIRE(ctx, "pg_xtable_destroy: ctx is NULL");
    if (!s) return PG_OK;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        std::unique_lock<std::shared_mutex> sw(s->rw);
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipDeviceSynchronize());
        pg::x2i_free_sides(s);
    }
    delete s;
    return PG_OK;
}

int pg_x2i_recall(pg_ctx* ctx, const pg_xtable* s, const uint32_t* trigger_rows, const double* trigger_prefer, const uint32_t* trigger_offsets,
                  uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count) {
    return pg::x2i_entry("pg_x2i_recall", ctx, s, trigger_rows, trigger_prefer, trigger_offsets, nq, k, opts, out_rows, out_scores, out_count, true);
}

int pg_x2i_recall_dev(pg_ctx* ctx, const pg_xtable* s, const uint32_t* d_trigger_rows, const double* d_trigger_prefer,
                      const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* d_out_rows,
                      double* d_out_scores, uint32_t* out_count) {
    return pg::x2i_entry("pg_x2i_recall_dev", ctx, s, d_trigger_rows, d_trigger_prefer, trigger_offsets, nq, k, opts, d_out_rows, d_out_scores,
                         out_count, false);
}

int pg_x2i_recall_host(uint64_t rows, uint64_t row_offset, uint32_t n_x, const uint64_t* i2x_off, const uint32_t* i2x_ids, const uint64_t* x2i_off,
                       const uint32_t* x2i_rows, const float* x2i_scores, const uint32_t* trigger_rows, const double* trigger_prefer,
                       const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* out_rows,
                       double* out_scores, uint32_t* out_count) {
    const char* who = "pg_x2i_recall_host";
    int rc;
    uint32_t nmax = 0;
    std::string err;
    PG_REQUIRE(i2x_off && x2i_off, "%s: NULL argument", who);
    PG_REQUIRE(rows >= 1 && rows < 0xFFFFFFFFull && n_x >= 1 && n_x < 0xFFFFFFFFu, "%s: rows=%llu, n_x=%u (1 .. 2^32 - 2 each)", who,
               (unsigned long long)rows, n_x);
    if ((rc = pg::x2i_check_args(who, trigger_rows, trigger_prefer, trigger_offsets, nq, k, opts, out_rows, out_scores, false, true, &nmax, &err)))
        return pg::x2i_fail(rc, err);
    // the CSR is held to what the uploads accept
    if (!pg::x2i_validate_lists(who, "row", "x id", 0, rows, i2x_off, i2x_ids, nullptr, pg::kX2iMaxXPerItem, n_x, &err) ||
        !pg::x2i_validate_lists(who, "X", "item row", 0, n_x, x2i_off, x2i_rows, x2i_scores, pg::kX2iMaxList, rows, &err))
        return pg::x2i_fail(PG_ERR_INVALID, err);
    PG_REQUIRE(x2i_off[n_x] == x2i_off[0] || x2i_scores, "%s: NULL argument", who);
    const uint32_t status = pg::x2i_recall_host(rows, row_offset, n_x, i2x_off, i2x_ids, x2i_off, x2i_rows, x2i_scores, trigger_rows, trigger_prefer,
                                                trigger_offsets, nq, k, opts, out_rows, out_scores, out_count);
    if (status != pg::kX2iNone) return pg::x2i_fail(PG_ERR_UNSUPPORTED, pg::x2i_limit_message(who, status));
    return PG_OK;
}

int pg_rtu2i_x_recall(pg_ctx* ctx, pg_rtu2i* c, const pg_xtable* s, const uint32_t* event_rows, const uint16_t* event_code,
                      const double* event_play_time, const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now, uint32_t nq,
                      uint32_t k, const pg_x2i_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count) {
    return pg::rt_x_recall_entry("pg_rtu2i_x_recall", ctx, c, s, event_rows, event_code, event_play_time, event_time, event_offsets, now, nq, k,
                                 opts, out_rows, out_scores, out_count, true);
}

int pg_rtu2i_x_recall_dev(pg_ctx* ctx, pg_rtu2i* c, const pg_xtable* s, const uint32_t* d_event_rows, const uint16_t* d_event_code,
                          const double* d_event_play_time, const int64_t* d_event_time, const uint32_t* event_offsets, const int64_t* now,
                          uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* d_out_rows, double* d_out_scores, uint32_t* out_count) {
    return pg::rt_x_recall_entry("pg_rtu2i_x_recall_dev", ctx, c, s, d_event_rows, d_event_code, d_event_play_time, d_event_time, event_offsets,
                                 now, nq, k, opts, d_out_rows, d_out_scores, out_count, false);
}

}  // extern "C"
