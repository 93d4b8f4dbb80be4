// traffic.hip — TrafficControlSort's macro control on the device: the reference's re-ranking behind the PID
// controller (sort/traffic_control_sort.go: macroControl :204-364, computeDeltaRank :555-589, the closing position sort :160-181).
// The controller stays on the host and hands over one alpha per target and request; include/pairec_gpu.h states the answer step
// by step (pg_traffic_sort_dev) and traffic_host.hpp holds every function of it that both sides run; the numbers of the steps
// below are the header's.
//
//   traffic_control_kernel  one workgroup of 1 024 lanes per request.  It resolves the request's alphas first: with every one 0 the
//                           passes below only compact the list and write the identity.  Pass 1 walks the list 1 024 entries at a time: a lane takes
//                           entry j, its element (through d_order) and, when that is an element of the arrays, its rank among the
//                           chunk's such entries (block_rank.hpp's chunk_rank) — its list index i — then
//                           s_i and w_i = s_i * posWeight_i; w_i and the member byte go to LDS at the rank, the element to the
//                           compacted list in scratch, its bit into the "is an entry" bitmap.  Lanes 0 .. T of wave 0 then each
//                           run ONE sequential chain over the chunk's staged values: lane 0 `total`, lane 1 + t `sum_t` and its
//                           "received an addition" flag (step 4: the chains are the reference's and fp64 addition is not
//                           associative, so nothing here is a tree).  Behind the last chunk lane t finishes target t
//                           (traffic_target: weight, scaled alpha, rho, the page-2 start) into LDS.  Pass 2: all lanes take
//                           entries again, steps 6 and 7 from the tables in global memory, new_pos and control_id by element,
//                           new_pos by list index into the key array (NaN behind the list: it sorts last).  Last, the elements
//                           that are no entry receive the padding values from the bitmap: every element is written once.
//   the order               sort_dev_locked (sort.hip), ascending, over nq segments of cap keys: ties keep the input order and
//                           NaN sorts last, which is step 8; the padding keys sit behind every entry's key, NaN or not.
//   traffic_compose_kernel  sorted list index → element through the compacted list; UINT32_MAX behind the count; the counts.
#include "pipeline.hpp"
#include "block_rank.hpp"
#include "cond_eval.hpp"      // SetTable
#include "traffic_host.hpp"

#include <cstdarg>
#include <memory>

namespace pg {
namespace {

constexpr uint32_t kTrafficChunk = 1024, kTrafficWaves = kTrafficChunk / kWave, kTrafficComposeThreads = 256;
constexpr uint32_t kTrafficEmpty = 0xFFFFFFFFu;
static_assert(kTrafficChunk == PG_TRIM_CHUNK, "include/pairec_gpu.h names the chunk");
static_assert(kTrafficMaxTargets + 1 <= (uint32_t)kWave, "the chains are lanes of one wave");
static_assert(kCandMaxCap / 32 == 512, "the bitmap of elements is 2 KB");

struct TrafficArgs {
    int32_t control_type[kTrafficMaxTargets], target_id[kTrafficMaxTargets];
    uint32_t T, cap;
    TrafficScalars sc;
    const double* tab;                     // the four tables (traffic_tables' layout)
    const double* score;                   // [nq][cap] by element
    const uint8_t* member;                 // [nq][cap] by element
    const uint32_t* order;                 // [nq][cap] list entry → element, or nullptr
    const uint32_t* count;                 // [nq] or nullptr
    const double* alpha;                   // [nq][T]
    double* key;                           // [nq][cap] new_pos by list index, NaN behind the list
    uint32_t* elems;                       // [nq][cap] the compacted list: list index → element
    uint32_t* n_list;                      // [nq] its length
    const uint32_t* sorted;                // [nq][cap] the keys' order (the compose kernel's)
    uint32_t* out_order;                   // [nq][cap]
    uint32_t* out_count;                   // [nq]
    int32_t* out_control_id;               // [nq][cap] by element, or nullptr
    double* out_new_pos;                   // [nq][cap] by element, or nullptr
};

// Request q = blockIdx.x.
__global__ __launch_bounds__(kTrafficChunk) void traffic_control_kernel(TrafficArgs a) {
    __shared__ __attribute__((aligned(16))) double s_w[kTrafficChunk];   // the chunk's w_i, by rank
    __shared__ __attribute__((aligned(16))) uint8_t s_m[kTrafficChunk];  // ... and member bytes
    __shared__ uint32_t s_isentry[kCandMaxCap / 32];                   // bit e: element e is an entry of the list
    __shared__ uint32_t s_wcnt[2 * kTrafficWaves];
    __shared__ double s_max;                                           // maxScore = s_0
    __shared__ TrafficTarget s_tg[kTrafficMaxTargets];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const size_t q0 = (size_t)q * a.cap;
    const uint32_t n = a.count ? min(a.count[q], a.cap) : a.cap, T = a.T;
    const uint32_t* ord = a.order ? a.order + q0 : nullptr;
    const double* alpha_q = a.alpha + (size_t)q * T;                   // (T = 0: never read)
    uint32_t* elems = a.elems + q0;
    for (uint32_t w = tid; w < kCandMaxCap / 32; w += kTrafficChunk) s_isentry[w] = 0;
    // 1. the request's alphas first: with every one 0 (or no target) nothing below reads a score, adds a chain or looks anything up
    bool live = false;
    for (uint32_t t = 0; t < T; ++t) live = live || alpha_q[t] != 0;
    // this lane's chain: lane 0 of wave 0 adds `total`, lane 1 + t `sum_t` when alpha_t != 0 (step 4)
    const bool chain = wave == 0 && lane <= T && live;
    const uint32_t my_t = lane ? lane - 1u : 0u;
    const bool chain_on = chain && (lane == 0 || alpha_q[my_t] != 0);
    double acc = 0.0;
    uint32_t seen = 0;                                                 // the OR of the member bytes the chain walked (in every byte lane)
    __syncthreads();

    // pass 1: compact, stage, add
    uint32_t run = 0, it = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += kTrafficChunk) {
        const uint32_t j = c0 + tid;
        const uint32_t elem = j < n ? (ord ? ord[j] : j) : a.cap;
        const bool valid = elem < a.cap;                               // (an order value outside the arrays leaves the list)
        uint32_t r, cnt;                                               // (r < cnt <= 1 024 where valid)
        chunk_rank<kTrafficWaves>(valid, s_wcnt, it++, &r, &cnt);      // its barrier also: the chains are done with the previous chunk's s_w / s_m
        if (live && tid >= cnt && tid < ((cnt + 7u) & ~7u)) {          // the chains read whole groups of eight slots
            s_w[tid] = -0.0;
            s_m[tid] = 0;
        }
        if (valid) {
            const uint32_t i = run + r;                                // i < n <= cap
            elems[i] = elem;
            atomicOr(&s_isentry[elem >> 5], 1u << (elem & 31u));
            if (live) {
                const double s = traffic_s(a.score[q0 + elem]);
                if (i == 0) s_max = s;
                s_w[r] = s * traffic_pos_weight(a.tab, i);
                s_m[r] = a.member[q0 + elem];
            }
        }
        __syncthreads();
        if (chain_on) {
            // (one loop for all chains, so that the wave walks the chunk once; one wave on its SIMD hides nothing, so the loop is
            // counted in instructions.  Eight staged values are read before the first of their adds: the LDS latency is paid once
            // per eight links.  A link is a mask test, a select and the add — x + -0.0 is x for every x, -0.0 and NaN included,
            // so the select stays off the chain of dependent adds.  The slots behind cnt up to the next multiple of eight hold
            // -0.0 and no member bit, so the loop has no tail; lane 0 tests nothing and takes every slot.)
            const uint32_t bit = lane ? 1u << my_t : 0u, never = lane ? 0u : 1u;
            for (uint32_t r0 = 0; r0 < cnt; r0 += 8) {
                double w[8];
#pragma unroll
                for (uint32_t u = 0; u < 8; u += 2) {
                    const double2 p = *reinterpret_cast<const double2*>(&s_w[r0 + u]);
                    w[u] = p.x;
                    w[u + 1] = p.y;
                }
                const uint2 mw = *reinterpret_cast<const uint2*>(&s_m[r0]);
                seen |= mw.x | mw.y;
#pragma unroll
                for (uint32_t u = 0; u < 8; ++u) {
                    const uint32_t bits = (u < 4 ? mw.x : mw.y) >> (8 * (u & 3u));       // (bit < 256 picks from the slot's own byte)
                    acc = acc + ((bits & bit) != never ? w[u] : -0.0);
                }
            }
        }
        run += cnt;
    }
    const uint32_t nl = run;                                           // the list's length
    // the targets' numbers: lane 1 + t holds sum_t, lane 0 total
    if (wave == 0 && live) {
        const double total = __shfl(acc, 0);
        seen |= seen >> 16;
        seen |= seen >> 8;
        if (lane >= 1 && lane <= T) s_tg[my_t] = traffic_target(a.tab, a.sc, alpha_q[my_t], acc, total, chain_on && ((seen >> my_t) & 1u) != 0);
    }
    __syncthreads();

    // pass 2: steps 6 and 7
    const double max_score = (live && nl) ? s_max : 0.0;
    double* key = a.key + q0;
    for (uint32_t i = tid; i < a.cap; i += kTrafficChunk) {
        if (i >= nl) {
            key[i] = traffic_nan();
            continue;
        }
        const uint32_t elem = elems[i];                                // (written by this workgroup before the barriers above)
        int32_t cid = (int32_t)(i + 1);
        double pos = (double)(i + 1);
        if (live) {
            const double s = traffic_s(a.score[q0 + elem]);
            traffic_entry(a.tab, s_tg, a.control_type, a.target_id, T, i, traffic_item_score(a.tab, i, s, max_score), a.member[q0 + elem], &cid, &pos);
        }
        key[i] = pos;
        if (a.out_control_id) a.out_control_id[q0 + elem] = cid;
        if (a.out_new_pos) a.out_new_pos[q0 + elem] = pos;
    }
    // the elements that are no entry
    if (a.out_control_id || a.out_new_pos)
        for (uint32_t e = tid; e < a.cap; e += kTrafficChunk)
            if (!((s_isentry[e >> 5] >> (e & 31u)) & 1u)) {
                if (a.out_control_id) a.out_control_id[q0 + e] = 0;
                if (a.out_new_pos) a.out_new_pos[q0 + e] = traffic_nan();
            }
    if (tid == 0) a.n_list[q] = nl;
}

// Request q = blockIdx.y, output slots blockIdx.x * 256 ...
__global__ __launch_bounds__(kTrafficComposeThreads) void traffic_compose_kernel(TrafficArgs a) {
    const uint32_t q = blockIdx.y, k = blockIdx.x * kTrafficComposeThreads + threadIdx.x;
    if (k >= a.cap) return;
    const size_t q0 = (size_t)q * a.cap;
    const uint32_t nl = a.n_list[q];
    uint32_t e = kTrafficEmpty;
    if (k < nl) {
        const uint32_t i = a.sorted[q0 + k];                           // (i < nl: the padding keys sort behind every entry's)
        e = i < nl ? a.elems[q0 + i] : kTrafficEmpty;
    }
    a.out_order[q0 + k] = e;
    if (k == 0) a.out_count[q] = nl;
}

}  // namespace
}  // namespace pg

// ---- the compiled object ------------------------------------------------------------------------------------------------------
struct pg_traffic {
    std::vector<pg_traffic_target> targets;
    pg::SetTable table;                               // the four tables
};

namespace pg {
namespace {

int traffic_refuse(int code, const char* who, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int traffic_refuse(int code, const char* who, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error("%s: %s", who, buf);
    return code;
}

int traffic_check_call(const pg_traffic* m, uint32_t ctx_size, uint32_t page_no, uint32_t nq, uint32_t cap, const void* score, const void* member,
                       const void* alpha, const char* who) {
    if (nq < 1 || nq > (uint32_t)kMaxQueries) return traffic_refuse(nq < 1 ? PG_ERR_INVALID : PG_ERR_UNSUPPORTED, who, "nq=%u must be in [1,%d]", nq, kMaxQueries);
    if (cap < 1 || cap > kCandMaxCap) return traffic_refuse(PG_ERR_UNSUPPORTED, who, "cap=%u unsupported (1..%u)", cap, kCandMaxCap);
    if (ctx_size == 0) return traffic_refuse(PG_ERR_INVALID, who, "ctx_size is 0 (ctx.Size: the page's size)");
    if (page_no == 0) return traffic_refuse(PG_ERR_INVALID, who, "page_no is 0 (the reference clamps page_number to 1: pass 1)");
    if (!m->targets.empty() && !(score && member && alpha))
        return traffic_refuse(PG_ERR_INVALID, who, "the set has %zu targets: score, member and alpha are needed", m->targets.size());
    return PG_OK;
}

void traffic_set_args(const pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta, int32_t* control_type,
                      int32_t* target_id, TrafficScalars* sc) {
    for (size_t t = 0; t < m->targets.size(); ++t) {
        control_type[t] = m->targets[t].control_type;
        target_id[t] = m->targets[t].target_id;
    }
    *sc = TrafficScalars{ctx_size, page_no, gamma, beta, eta};
}

// launches; caller holds ctx->mu.  d_* as pg_traffic_sort_dev takes them.
int traffic_sort_locked(pg_ctx* ctx, pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta, uint32_t nq,
                        uint32_t cap, const double* d_score, const uint8_t* d_member, const uint32_t* d_order, const uint32_t* d_count,
                        const double* d_alpha, uint32_t* d_out_order, uint32_t* d_out_count, int32_t* d_out_control_id, double* d_out_new_pos,
                        const char* who) {
    int rc;
    TrafficArgs a{};
    traffic_set_args(m, ctx_size, page_no, gamma, beta, eta, a.control_type, a.target_id, &a.sc);
    a.T = (uint32_t)m->targets.size();
    a.cap = cap;
    if ((rc = m->table.ensure(ctx, who, {{traffic_tables(), (size_t)kTrafficTableN * 8}}))) return rc;
    a.tab = m->table.part<double>(0);
    a.score = d_score;
    a.member = d_member;
    a.order = d_order;
    a.count = d_count;
    a.alpha = d_alpha;
    uint32_t *d_off = nullptr, *d_sorted = nullptr;
    if ((rc = scratch_carve(ctx, kSlotTraffic, [&](Carve& c) {
            a.key = c.take<double>((size_t)nq * cap);
            a.elems = c.take<uint32_t>((size_t)nq * cap);
            d_sorted = c.take<uint32_t>((size_t)nq * cap);
            a.n_list = c.take<uint32_t>(nq);
            d_off = c.take<uint32_t>((size_t)nq + 1);
        }))) return rc;
    a.sorted = d_sorted;
    a.out_order = d_out_order;
    a.out_count = d_out_count;
    a.out_control_id = d_out_control_id;
    a.out_new_pos = d_out_new_pos;
    traffic_control_kernel<<<nq, kTrafficChunk, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    if ((rc = uniform_offsets_locked(ctx, nq, cap, d_off))) return rc;
    if ((rc = sort_dev_locked(ctx, a.key, d_off, nq, nq * cap, cap, 0, d_sorted))) return rc;
    traffic_compose_kernel<<<dim3((cap + kTrafficComposeThreads - 1) / kTrafficComposeThreads, nq), kTrafficComposeThreads, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_traffic_compile(const pg_traffic_target* targets, uint32_t n, pg_traffic** out) {
    const char* who = "pg_traffic_compile";
    PG_REQUIRE(out && (n == 0 || targets), "pg_traffic_compile: NULL argument");
    if (n > pg::kTrafficMaxTargets) return pg::traffic_refuse(PG_ERR_UNSUPPORTED, who, "%u targets (at most %u: a member mask is one byte)", n, pg::kTrafficMaxTargets);
    for (uint32_t t = 0; t < n; ++t) {
        if (targets[t].control_type != PG_TRAFFIC_PERCENT && targets[t].control_type != PG_TRAFFIC_QUANTITY)
            return pg::traffic_refuse(PG_ERR_UNSUPPORTED, who, "target %u: unknown control type %d (PG_TRAFFIC_PERCENT or PG_TRAFFIC_QUANTITY)", t, targets[t].control_type);
        if (targets[t].target_id == INT32_MIN)
            return pg::traffic_refuse(PG_ERR_INVALID, who, "target %u: target_id %d has no negation in int32 (a Percent target's control id is -target_id)", t, targets[t].target_id);
    }
    std::unique_ptr<pg_traffic> m(new pg_traffic());
    m->targets.assign(targets, targets + n);
    *out = m.release();
    return PG_OK;
}

int pg_traffic_free(pg_traffic* m) {
    if (!m) return PG_OK;
    m->table.release();
    delete m;
    return PG_OK;
}

int pg_traffic_num_targets(const pg_traffic* m) { return m ? (int)m->targets.size() : 0; }

int pg_traffic_table(int which, uint32_t first, uint32_t n, double* out) {
    static const uint32_t at[4] = {pg::kTrafficPosAt, pg::kTrafficExpAt, pg::kTrafficTanhAt, pg::kTrafficSigAt};
    static const uint32_t len[4] = {pg::kTrafficPosN, pg::kTrafficExpN, pg::kTrafficTanhN, pg::kTrafficSigN};
    PG_REQUIRE(which >= 0 && which < 4, "pg_traffic_table: table %d (0 positionWeight, 1 expTable, 2 tanhTable, 3 sigmoidTable)", which);
    PG_REQUIRE(first <= len[which] && n <= len[which] - first, "pg_traffic_table: entries [%u, %u + %u) of a table of %u", first, first, n, len[which]);
    PG_REQUIRE(out || n == 0, "pg_traffic_table: NULL argument");
    if (n) memcpy(out, pg::traffic_tables() + at[which] + first, (size_t)n * 8);
    return PG_OK;
}

int pg_traffic_sort_host(const pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta, uint32_t nq,
                         uint32_t cap, const double* score, const uint8_t* member, const uint32_t* order, const uint32_t* count,
                         const double* alpha, uint32_t* out_order, uint32_t* out_count, int32_t* out_control_id, double* out_new_pos) {
    const char* who = "pg_traffic_sort_host";
    PG_REQUIRE(m && out_order && out_count, "pg_traffic_sort_host: NULL argument");
    int rc;
    if ((rc = pg::traffic_check_call(m, ctx_size, page_no, nq, cap, score, member, alpha, who))) return rc;
    const uint32_t T = (uint32_t)m->targets.size();
    for (uint32_t q = 0; order && q < nq; ++q) {
        const uint32_t n = count ? std::min(count[q], cap) : cap;
        for (uint32_t j = 0; j < n; ++j)
            if (order[(size_t)q * cap + j] >= cap)
                return pg::traffic_refuse(PG_ERR_INVALID, who, "order[%u][%u] = %u is no element of the arrays (cap %u)", q, j, order[(size_t)q * cap + j], cap);
    }
    int32_t control_type[pg::kTrafficMaxTargets] = {0}, target_id[pg::kTrafficMaxTargets] = {0};
    pg::TrafficScalars sc;
    pg::traffic_set_args(m, ctx_size, page_no, gamma, beta, eta, control_type, target_id, &sc);
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t q0 = (size_t)q * cap;
        const uint32_t n = count ? std::min(count[q], cap) : cap;
        pg::traffic_host_request(sc, control_type, target_id, T, n, cap, score ? score + q0 : nullptr, member ? member + q0 : nullptr,
                                 order ? order + q0 : nullptr, alpha ? alpha + (size_t)q * T : nullptr, out_order + q0, out_count + q,
                                 out_control_id ? out_control_id + q0 : nullptr, out_new_pos ? out_new_pos + q0 : nullptr);
    }
    return PG_OK;
}

int pg_traffic_sort_dev(pg_ctx* ctx, pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta,
                        uint32_t nq, uint32_t cap, const double* d_score, const uint8_t* d_member, const uint32_t* d_order,
                        const uint32_t* d_count, const double* d_alpha, uint32_t* d_out_order, uint32_t* d_out_count,
                        int32_t* d_out_control_id, double* d_out_new_pos) {
    const char* who = "pg_traffic_sort_dev";
    PG_REQUIRE(ctx && m && d_out_order && d_out_count, "pg_traffic_sort_dev: NULL argument");
    int rc;
    if ((rc = pg::traffic_check_call(m, ctx_size, page_no, nq, cap, d_score, d_member, d_alpha, who))) return rc;
    const size_t e = (size_t)nq * cap, T = m->targets.size();
    const struct { const void* p; size_t bytes; const char* name; } ins[] = {{d_score, e * 8, "d_score"}, {d_member, e, "d_member"},
        {d_order, e * 4, "d_order"}, {d_count, (size_t)nq * 4, "d_count"}, {d_alpha, (size_t)nq * T * 8, "d_alpha"}},
      outs[] = {{d_out_order, e * 4, "d_out_order"}, {d_out_count, (size_t)nq * 4, "d_out_count"}, {d_out_control_id, e * 4, "d_out_control_id"},
                {d_out_new_pos, e * 8, "d_out_new_pos"}};
    for (size_t o = 0; o < 4; ++o) {
        for (const auto& in : ins)
            PG_REQUIRE(!in.bytes || !pg::cand_overlap(in.p, in.bytes, outs[o].p, outs[o].bytes), "pg_traffic_sort_dev: %s overlaps %s", outs[o].name, in.name);
        for (size_t o2 = o + 1; o2 < 4; ++o2)
            PG_REQUIRE(!pg::cand_overlap(outs[o2].p, outs[o2].bytes, outs[o].p, outs[o].bytes), "pg_traffic_sort_dev: %s overlaps %s", outs[o].name, outs[o2].name);
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::traffic_sort_locked(ctx, m, ctx_size, page_no, gamma, beta, eta, nq, cap, d_score, d_member, d_order, d_count, d_alpha, d_out_order,
                                   d_out_count, d_out_control_id, d_out_new_pos, who);
}

// ---- one request on host arrays (staged_run, cand_lists.hpp) ---------------------------------------------------------------------
int pg_traffic_sort(pg_ctx* ctx, pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta, uint32_t n,
                    const double* score, const uint8_t* member, const uint32_t* order, const double* alpha, uint32_t* out_order,
                    uint32_t* out_count, int32_t* out_control_id, double* out_new_pos) {
    const char* who = "pg_traffic_sort";
    PG_REQUIRE(ctx && m && out_count && (n == 0 || out_order), "pg_traffic_sort: NULL argument");
    if (n == 0) {                                    // an empty request: an empty answer
        *out_count = 0;
        return PG_OK;
    }
    int rc;
    if ((rc = pg::traffic_check_call(m, ctx_size, page_no, 1, n, score, member, alpha, who))) return rc;
    for (uint32_t j = 0; order && j < n; ++j)
        if (order[j] >= n) return pg::traffic_refuse(PG_ERR_INVALID, who, "order[%u] = %u is no element of the arrays (n %u)", j, order[j], n);
    const size_t T = m->targets.size();
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kScore, kNewPos, kAlpha, kOrder, kOutOrder, kControl, kCount, kMember };
    Staged st[] = {{score, (size_t)n * 8, Staged::in_if(T ? score : nullptr)},
                   {out_new_pos, (size_t)n * 8, Staged::out_if(out_new_pos)},
                   {alpha, T * 8, Staged::in_if(T ? alpha : nullptr), pg::kTrafficMaxTargets * 8},
                   {order, (size_t)n * 4, Staged::in_if(order)},
                   {out_order, (size_t)n * 4, Staged::kOut},
                   {out_control_id, (size_t)n * 4, Staged::out_if(out_control_id)},
                   {out_count, 4, Staged::kOut},
                   {member, n, Staged::in_if(T ? member : nullptr)}};
    return pg::staged_run(ctx, pg::kSlotStaging, st, sizeof st / sizeof *st, false, [&] {
        return pg::traffic_sort_locked(ctx, m, ctx_size, page_no, gamma, beta, eta, 1, n, T ? st[kScore].at<double>() : nullptr,
                                       T ? st[kMember].at<uint8_t>() : nullptr, order ? st[kOrder].at<uint32_t>() : nullptr, nullptr,
                                       T ? st[kAlpha].at<double>() : nullptr, st[kOutOrder].at<uint32_t>(), st[kCount].at<uint32_t>(),
                                       out_control_id ? st[kControl].at<int32_t>() : nullptr, out_new_pos ? st[kNewPos].at<double>() : nullptr, who);
    });
}

}  // extern "C"
