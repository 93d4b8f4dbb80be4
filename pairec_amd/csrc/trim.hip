// trim.hip — a request's merged candidates cut down on the device: recall quotas and the coarse-rank cut.
//
// Between UniqueFilter and RankService.Rank (service/user_recommend.go:105-137) two stages shorten the union of a request's
// recalls: PriorityAdjustCountFilter (filter/priority_adjust_count_filter.go:80-251) sorts it by Item.Score, groups it by
// RetrieveId and keeps a quota per recall in the order the config names them; GeneralRank's actions
// (service/general_rank/action.go:61-83) sort by the coarse score and keep the first RetainNum (filter/adjust_count_filter.go:58-71).
// Both are one primitive: order a request's list by a score, keep the first n_c entries of each class of sources, class after
// class.  The order is the score sort's (sort.hip); this file's kernel turns it into the output permutation and gathers every
// carried array through it: one workgroup per request, no value meets arithmetic.
//   count   real entries per class (order does not matter: wave ballots added up in LDS);
//   plan    one lane turns the rules and the counts into each class's take and output base;
//   walk    the sorted order in chunks of kTrimChunk positions: an entry's rank within its class = the class's running count +
//           the entries of its class in the waves before it (per-wave class counts in LDS, two sets as block_rank.hpp's
//           chunk_rank keeps them) + those in the lanes before it (its ballot_rank); a rank below the class's take is written
//           at base[class] + rank;
//   pad     the slots behind the takes.
#include "pipeline.hpp"
#include "block_rank.hpp"

#include <algorithm>

namespace pg {
namespace {

constexpr uint32_t kTrimMaxRules = 8;
constexpr uint32_t kTrimMaxSources = 8;
constexpr uint32_t kTrimMaxPlanes = 8;
constexpr uint32_t kTrimMaxCap = 16384;
constexpr uint32_t kTrimChunk = 1024;            // positions walked at a time = the workgroup's lanes
static_assert(kTrimMaxRules == PG_TRIM_MAX_RULES && kTrimMaxSources == PG_TRIM_MAX_SOURCES && kTrimMaxPlanes == PG_TRIM_MAX_PLANES &&
                  kTrimMaxCap == PG_TRIM_MAX_CAP && kTrimChunk == PG_TRIM_CHUNK,
              "include/pairec_gpu.h repeats these");
static_assert(kTrimMaxSources == kCandMaxSources && kTrimMaxPlanes == kCandMaxPlanes && kTrimMaxCap == kCandMaxCap,
              "the header names the limits per stage; cand_lists.hpp holds them together");
constexpr uint32_t kTrimThreads = kTrimChunk;
constexpr uint32_t kTrimWaves = kTrimThreads / kWave;
constexpr uint32_t kTrimNone = 0xFFu;            // the class of padding and of entries whose source no rule names

struct TrimArgs {
    CandIn in;                                   // (source NULL: the single rule matches every source)
    CandOut out;
    const uint32_t* order;                       // [nq][cap]: each request's positions in score order
    uint32_t n_rules;
    uint32_t any;                                // the single rule is PG_TRIM_ANY
    uint32_t r_count[kTrimMaxRules];
    uint8_t r_source[kTrimMaxRules], r_type[kTrimMaxRules];
};

// the class (= rule index) of the entry at position p of the request, kTrimNone for padding and for sources no rule names
__device__ inline uint32_t trim_class(const TrimArgs& a, const uint32_t* cls_of, size_t in0, uint32_t p, uint32_t n_valid) {
    if (p >= n_valid || a.in.rows[in0 + p] == kCandPad) return kTrimNone;
    if (a.any) return 0u;
    const uint32_t s = a.in.source[in0 + p];
    return s < kTrimMaxSources ? cls_of[s] : kTrimNone;
}

// Request q = blockIdx.x.
__global__ __launch_bounds__(kTrimThreads) void candidates_trim_kernel(TrimArgs a) {
    __shared__ uint32_t cls_of[kTrimMaxSources], ccnt[kTrimMaxRules], take[kTrimMaxRules], base[kTrimMaxRules], run[kTrimMaxRules];
    __shared__ uint32_t wcnt[2][kTrimMaxRules][kTrimWaves];
    __shared__ uint32_t total_s;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t cap = a.in.cap, out_cap = a.out.out_cap, n_rules = a.n_rules;
    const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    if (tid < kTrimMaxSources) cls_of[tid] = kTrimNone;
    if (tid < kTrimMaxRules) {
        ccnt[tid] = 0;
        run[tid] = 0;
    }
    __syncthreads();
    if (tid == 0 && !a.any)
        for (uint32_t r = 0; r < n_rules; ++r) cls_of[a.r_source[r]] = r;        // (sources < kTrimMaxSources, each named once: the host checked)
    __syncthreads();
    // count: the real entries of every class
    for (uint32_t c0 = 0; c0 < cap; c0 += kTrimChunk) {
        const uint32_t p = c0 + tid;
        const uint32_t c = p < cap ? trim_class(a, cls_of, in0, p, n_valid) : kTrimNone;
        for (uint32_t r = 0; r < n_rules; ++r) {
            const unsigned long long m = __ballot(c == r);
            if (lane == 0 && m) atomicAdd(&ccnt[r], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    // plan: priority_adjust_count_filter.go:141-203 on the counts (FIX leaves the accumulator alone, :145-150)
    if (tid == 0) {
        uint32_t acc = 0, at = 0;
        for (uint32_t r = 0; r < n_rules; ++r) {
            const uint32_t len = ccnt[r], cnt = a.r_count[r];
            uint32_t t;
            if (a.r_type[r] == PG_TRIM_FIX) {
                t = min(len, cnt);
            } else {
                t = min(len, cnt > acc ? cnt - acc : 0u);
                acc += t;
            }
            take[r] = t;
            base[r] = at;
            at += t;
        }
        total_s = min(at, out_cap);                          // (at <= out_cap by pg_trim_out_cap's sum)
    }
    __syncthreads();
    // walk: the sorted order, chunk after chunk
    for (uint32_t c0 = 0, it = 0; c0 < cap; c0 += kTrimChunk, ++it) {
        const uint32_t i = c0 + tid;
        uint32_t pos = 0, c = kTrimNone;
        if (i < cap) {
            pos = a.order[in0 + i];
            if (pos < cap) c = trim_class(a, cls_of, in0, pos, n_valid);
        }
        uint32_t(*wc)[kTrimWaves] = wcnt[it & 1u];           // (two sets of counts: a wave ahead by one chunk writes the other one)
        uint32_t before = 0;
        for (uint32_t r = 0; r < n_rules; ++r) {
            const unsigned long long m = __ballot(c == r);
            if (c == r) before = ballot_rank(m);
            if (lane == 0) wc[r][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (c != kTrimNone) {
            uint32_t rank = run[c] + before;
            for (uint32_t w = 0; w < wave; ++w) rank += wc[c][w];
            const uint32_t dst = base[c] + rank;
            if (rank < take[c] && dst < out_cap) cand_carry(a.in, a.out, in0 + pos, out0 + dst, true);
        }
        __syncthreads();
        // (the running counts move between this chunk's reads and the next chunk's, which lie behind its barrier)
        if (tid < n_rules) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < kTrimWaves; ++w) s += wc[tid][w];
            run[tid] += s;
        }
    }
    // pad: every slot behind the takes
    const uint32_t total = total_s;
    cand_pad(a.in, a.out, q, total + tid, kTrimThreads, kCandNegInf);
    if (tid == 0) a.out.count[q] = total;
}

// the rules as the reference can run them (priority_adjust_count_filter.go:123,193-195) and the width of what they keep
int trim_check_rules(const pg_trim_rule* rules, uint32_t n_rules, uint32_t cap, uint32_t* out_cap, const char* who) {
    if (!rules || n_rules < 1) {
        set_error("%s: no rules (the reference indexes configs[len - 1])", who);
        return PG_ERR_INVALID;
    }
    if (n_rules > kTrimMaxRules) {
        set_error("%s: n_rules=%u unsupported (1..%u)", who, n_rules, kTrimMaxRules);
        return PG_ERR_UNSUPPORTED;
    }
    uint64_t fix = 0, acc = 0;
    uint32_t seen = 0;
    for (uint32_t r = 0; r < n_rules; ++r) {
        const pg_trim_rule& ru = rules[r];
        if (ru.type != PG_TRIM_FIX && ru.type != PG_TRIM_ACCUMULATE) {
            set_error("%s: rule %u has type %u (PG_TRIM_FIX or PG_TRIM_ACCUMULATE)", who, r, ru.type);
            return PG_ERR_INVALID;
        }
        if (ru.source == PG_TRIM_ANY) {
            if (n_rules != 1) {
                set_error("%s: rule %u is PG_TRIM_ANY beside other rules (it is only valid as the single rule)", who, r);
                return PG_ERR_INVALID;
            }
        } else if (ru.source >= kTrimMaxSources) {
            set_error("%s: rule %u names source %u (< %u, or PG_TRIM_ANY)", who, r, ru.source, kTrimMaxSources);
            return PG_ERR_INVALID;
        } else if ((seen >> ru.source) & 1u) {
            set_error("%s: source %u is named twice (the reference would emit its items twice)", who, ru.source);
            return PG_ERR_INVALID;
        } else {
            seen |= 1u << ru.source;
        }
        if (ru.type == PG_TRIM_FIX) {
            fix += ru.count;
        } else {
            if (ru.count < acc) {
                set_error("%s: rule %u accumulates to %u after %llu (the reference slices with a negative bound and panics)", who, r, ru.count,
                          (unsigned long long)acc);
                return PG_ERR_INVALID;
            }
            acc = ru.count;
        }
    }
    if (cap < 1 || cap > kTrimMaxCap) {
        set_error("%s: cap=%u unsupported (1..%u)", who, cap, kTrimMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    if (out_cap) *out_cap = (uint32_t)std::min<uint64_t>(cap, fix + acc);
    return PG_OK;
}

}  // namespace

// caller holds ctx->mu and has checked the arguments (trim_check_rules, the pointers); d_order: each request's positions in score
// order if the caller has them already, else NULL (the score sort runs here); no synchronisation
int candidates_trim_locked(pg_ctx* ctx, const pg_trim_rule* rules, uint32_t n_rules, const CandIn& in, const CandOut& out,
                           const uint32_t* d_order) {
    const uint32_t nq = in.nq, cap = in.cap;
    int rc;
    if (out.out_cap == 0) {                      // every count is 0: nothing is kept, nothing but the counts is written
        PG_HIP(hipMemsetAsync(out.count, 0, (size_t)nq * 4, ctx->stream));
        return PG_OK;
    }
    if (!d_order) {
        uint32_t *d_off, *d_ord;
        if ((rc = scratch_carve(ctx, kSlotTrim, [&](Carve& c) {
                d_off = c.take<uint32_t>((size_t)nq + 1);
                d_ord = c.take<uint32_t>((size_t)nq * cap);
            }))) return rc;
        if ((rc = uniform_offsets_locked(ctx, nq, cap, d_off))) return rc;
        // (what the sort makes of padding does not matter: the kernel skips padding wherever it lies in the order)
        if ((rc = sort_dev_locked(ctx, reinterpret_cast<const double*>(in.score), d_off, nq, nq * cap, cap, 1, d_ord))) return rc;
        d_order = d_ord;
    }
    TrimArgs a{};
    a.in = in;
    a.out = out;
    a.order = d_order;
    a.n_rules = n_rules;
    a.any = rules[0].source == PG_TRIM_ANY ? 1u : 0u;
    for (uint32_t r = 0; r < n_rules; ++r) {
        a.r_count[r] = rules[r].count;
        a.r_source[r] = rules[r].source;
        a.r_type[r] = rules[r].type;
    }
    candidates_trim_kernel<<<nq, kTrimThreads, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_trim_out_cap(const pg_trim_rule* rules, uint32_t n_rules, uint32_t cap, uint32_t* out_cap) {
    PG_REQUIRE(out_cap, "pg_trim_out_cap: NULL argument");
    return pg::trim_check_rules(rules, n_rules, cap, out_cap, "pg_trim_out_cap");
}

int pg_candidates_trim_dev(pg_ctx* ctx, const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                           const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                           uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                           double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                           float* d_out_planes_f32, uint32_t* d_out_count) {
    const char* who = "pg_candidates_trim_dev";
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    uint32_t out_cap = 0;
    int rc;
    if ((rc = pg::cand_call_required(l, ctx, who)) || (rc = pg::cand_check_nq(nq, who)) || (rc = pg::trim_check_rules(rules, n_rules, cap, &out_cap, who)))
        return rc;
    PG_REQUIRE(d_source || rules[0].source == PG_TRIM_ANY, "%s: rules that name sources need d_source", who);
    if ((rc = pg::cand_lists_check(l, pg::kTrimMaxPlanes, who))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::candidates_trim_locked(ctx, rules, n_rules, in, out, nullptr);
}

}  // extern "C"
