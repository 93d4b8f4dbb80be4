// trim2.hip — recall quotas over RecallScores on the device: PriorityAdjustCountFilterV2.
//
// The quota filter of a scene whose recalls overlap (filter/priority_adjust_count_filter_v2.go:39-103), in the trim's slot between
// UniqueFilter and RankService.Rank (service/user_recommend.go:105-137).  An item that several recalls returned (len(RecallScores)
// > 1, :55) stands in the list of every configured recall that holds it, keyed by that recall's score (:66-71), until one quota
// takes it; it leaves with that recall's name and score (:68-69) and is gone from every later list (:80-83,91-93) without using
// up a place there.  The trim (trim.hip) cannot say that: its classes partition the entries.  The orders are the score sort's
// (sort.hip); the kernels here turn them into the output permutation and gather every carried array through it: no value meets
// arithmetic.
//   keys    one key array per rule (members: the score or the recall's plane; everything else NaN), sorted as nq x n_rules
//           segments through the call the blend uses;
//   cut     one workgroup per request, rules one after another (a rule's limit and the taken entries need the rules before):
//           inside a rule the rule's order kTrim2Chunk positions at a time; a lane is eligible iff its position is a member
//           (recomputed from source / mask: the sort cannot tell a non-member from a member with a NaN key) and its bit in the
//           LDS bitmap of input positions is clear; its rank = the rule's picks so far + its rank among the chunk's eligibles
//           (block_rank.hpp's chunk_rank); rank < limit: written at base + rank, bit set.
//           A rule's walk ends with the chunk in which its picks reach the limit, or with the order — never at a chunk without an
//           eligible entry: an earlier rule may have taken the first kTrim2Chunk members of this one's list;
//   pad     the slots behind the picks.
// pg_candidates_trim2_host states the same answer on host arrays with plain containers; the tests hold the device to it.
#include "pipeline.hpp"
#include "block_rank.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace pg {
namespace {

constexpr uint32_t kTrim2MaxRules = 8;
constexpr uint32_t kTrim2Chunk = 1024;           // positions walked at a time = the workgroup's lanes
static_assert(kTrim2MaxRules == PG_TRIM_MAX_RULES && kTrim2Chunk == PG_TRIM_CHUNK, "include/pairec_gpu.h: the trim's limits are this call's");
static_assert(kCandMaxSources == PG_TRIM_MAX_SOURCES && kCandMaxPlanes == PG_TRIM_MAX_PLANES && kCandMaxCap == PG_TRIM_MAX_CAP,
              "cand_lists.hpp holds the limits of the lists");
constexpr uint32_t kTrim2Waves = kTrim2Chunk / kWave;
static_assert(kCandMaxCap % 32 == 0, "the bitmap of taken positions is whole words");

struct Trim2Args {
    CandIn in;                                   // (source NULL: the single rule owns every entry)
    CandOut out;
    const uint32_t* order;                       // [nq][n_rules][cap]: positions in score order of each rule's keys
    uint32_t n_rules;
    uint32_t r_count[kTrim2MaxRules];
    uint8_t r_source[kTrim2MaxRules], r_type[kTrim2MaxRules];
};

// Is the entry at index e (= q * cap + p, p < cap) a member of the list of the rule that names source sc, and is its key there
// the recall's plane (else d_score)?  (priority_adjust_count_filter_v2.go:54-71)
__host__ __device__ __forceinline__ bool trim2_member(const CandIn& in, size_t e, uint32_t p, uint32_t n_valid, uint32_t sc, bool* plane) {
    *plane = false;
    if (p >= n_valid || in.rows[e] == kCandPad) return false;
    const uint32_t m = in.mask ? in.mask[e] : 0u;
    const bool dup = __builtin_popcount(m) > 1;       // (len(RecallScores) > 1, :55)
    if (dup) {                                   // RecallScores[name] is read for every name, its own source's too (:66-71)
        *plane = ((m >> sc) & 1u) != 0;
        return *plane;
    }
    return !in.source || in.source[e] == sc;     // (no source: every entry is of the single rule's)
}

__host__ __device__ __forceinline__ unsigned long long trim2_key(const CandIn& in, size_t e, uint32_t sc, bool plane) {
    return plane ? in.planes64[(size_t)sc * in.nq * in.cap + e] : in.score[e];
}

// keys: key[q][c][p] = the key of position p in rule c's list, NaN where it is no member (it sorts behind every number; the cut
// recomputes the membership)
__global__ __launch_bounds__(256) void trim2_keys_kernel(Trim2Args a, unsigned long long* keys) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x, c = blockIdx.y, q = blockIdx.z;
    const uint32_t cap = a.in.cap;
    if (p >= cap) return;
    const size_t e = (size_t)q * cap + p;
    const uint32_t sc = a.r_source[c];
    bool plane;
    unsigned long long k = kCandNan;
    if (trim2_member(a.in, e, p, cand_n_valid(a.in, q), sc, &plane)) k = trim2_key(a.in, e, sc, plane);
    keys[((size_t)q * a.n_rules + c) * cap + p] = k;
}

// cut: request q = blockIdx.x.
__global__ __launch_bounds__(kTrim2Chunk) void candidates_trim2_kernel(Trim2Args a) {
    __shared__ uint32_t taken[kCandMaxCap / 32];                     // one bit per input position: an earlier pick
    __shared__ uint32_t wcnt[2 * kTrim2Waves];                       // a chunk's eligible entries per wave
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t cap = a.in.cap, out_cap = a.out.out_cap, n_rules = a.n_rules;
    const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    for (uint32_t w = tid; w < kCandMaxCap / 32; w += kTrim2Chunk) taken[w] = 0u;
    __syncthreads();
    // the accumulator, the picks so far and every loop condition: each lane computes them from the same LDS words
    uint32_t acc = 0, base = 0, it = 0;
    for (uint32_t c = 0; c < n_rules; ++c) {
        const uint32_t cnt = a.r_count[c], sc = a.r_source[c];
        const uint32_t limit = a.r_type[c] == PG_TRIM_FIX ? cnt : (cnt > acc ? cnt - acc : 0u);
        const size_t l0 = ((size_t)q * n_rules + c) * cap;
        uint32_t picks = 0;                                          // rule c's picks in the chunks before
        for (uint32_t c0 = 0; c0 < cap && picks < limit; c0 += kTrim2Chunk, ++it) {
            const uint32_t i = c0 + tid;
            uint32_t pos = 0;
            bool elig = false, plane = false;
            if (i < cap) {
                pos = a.order[l0 + i];
                if (pos < cap)
                    elig = trim2_member(a.in, in0 + pos, pos, n_valid, sc, &plane) && !((taken[pos >> 5] >> (pos & 31u)) & 1u);
            }
            uint32_t r, total;
            chunk_rank<kTrim2Waves>(elig, wcnt, it, &r, &total);
            const uint32_t rank = picks + r;
            if (elig && rank < limit) {
                const uint32_t dst = base + rank;
                if (dst < out_cap) {                                 // (always: pg_trim2_out_cap's bound)
                    const size_t src = in0 + pos, o = out0 + dst;
                    cand_carry(a.in, a.out, src, o, false);
                    a.out.score[o] = trim2_key(a.in, src, sc, plane);                // (:68-69: the rule's name and its score)
                    if (a.out.source) a.out.source[o] = (uint8_t)sc;
                }
                // (the order is a permutation: no lane reads this bit again inside this rule; the OR does not depend on arrival order)
                atomicOr(&taken[pos >> 5], 1u << (pos & 31u));
            }
            picks += min(total, limit - picks);
        }
        if (a.r_type[c] != PG_TRIM_FIX) acc += picks;
        base += picks;
        __syncthreads();                                             // the rule's bits are set before the next rule reads the bitmap
    }
    const uint32_t total = min(base, out_cap);
    cand_pad(a.in, a.out, q, total + tid, kTrim2Chunk, kCandNegInf);
    if (tid == 0) a.out.count[q] = total;
}

// the rules as V2 can run them and the width of what they keep
int trim2_check_rules(const pg_trim_rule* rules, uint32_t n_rules, uint32_t cap, uint32_t* out_cap, const char* who) {
    if (!rules || n_rules < 1) {
        set_error("%s: no rules (AdjustCountConfs is empty)", who);
        return PG_ERR_INVALID;
    }
    if (n_rules > kTrim2MaxRules) {
        set_error("%s: n_rules=%u unsupported (1..%u)", who, n_rules, kTrim2MaxRules);
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
            set_error("%s: rule %u is PG_TRIM_ANY (V2 reads RecallScores by recall name: every rule names a source)", who, r);
            return PG_ERR_INVALID;
        }
        if (ru.source >= kCandMaxSources) {
            set_error("%s: rule %u names source %u (< %u)", who, r, ru.source, kCandMaxSources);
            return PG_ERR_INVALID;
        }
        if ((seen >> ru.source) & 1u) {
            set_error("%s: source %u is named twice (the reference would emit its items twice)", who, ru.source);
            return PG_ERR_INVALID;
        }
        seen |= 1u << ru.source;
        if (ru.type == PG_TRIM_FIX) fix += ru.count;
        else acc = std::max<uint64_t>(acc, ru.count);                // (a smaller count after a larger one is legal: :86-88 compares)
    }
    if (cap < 1 || cap > kCandMaxCap) {
        set_error("%s: cap=%u unsupported (1..%u)", who, cap, kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    if (out_cap) *out_cap = (uint32_t)std::min<uint64_t>(cap, fix + acc);
    return PG_OK;
}

// the checks both entry points share, in the order they fire: the pointers, nq, the rules, the pairs of optional arrays, what
// the rules and the mask need of them, the overlaps
int trim2_check_call(const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const CandCall& l, uint32_t* out_cap, const char* who) {
    int rc;
    if ((rc = cand_call_required(l, true, who)) || (rc = cand_check_nq(nq, who)) || (rc = trim2_check_rules(rules, n_rules, cap, out_cap, who)) ||
        (rc = cand_lists_check(l, kCandMaxPlanes, who)))
        return rc;
    PG_REQUIRE(l.source || n_rules == 1, "%s: rules that name more than one source need d_source", who);
    if (l.source_mask) {
        uint32_t need = 0;
        for (uint32_t r = 0; r < n_rules; ++r) need = std::max(need, (uint32_t)rules[r].source + 1u);
        PG_REQUIRE(l.planes_f64 && l.n_f64 >= need, "%s: a source mask needs the per-recall score planes of every named source (n_f64 >= %u)", who,
                   need);
    }
    return cand_call_apart(l, nq, cap, *out_cap, who);
}

}  // namespace

// caller holds ctx->mu and has checked the arguments (trim2_check_call); no synchronisation
int candidates_trim2_locked(pg_ctx* ctx, const pg_trim_rule* rules, uint32_t n_rules, const CandIn& in, const CandOut& out) {
    const uint32_t nq = in.nq, cap = in.cap, n_seg = nq * n_rules;
    int rc;
    if (out.out_cap == 0) {                      // every count is 0: nothing is kept, nothing but the counts is written
        PG_HIP(hipMemsetAsync(out.count, 0, (size_t)nq * 4, ctx->stream));
        return PG_OK;
    }
    // scratch: segment offsets | orders | keys
    uint32_t *d_off, *d_ord; unsigned long long* d_keys;
    if ((rc = scratch_carve(ctx, kSlotTrim2, [&](Carve& c) {
            d_off = c.take<uint32_t>((size_t)n_seg + 1);
            d_ord = c.take<uint32_t>((size_t)n_seg * cap);
            d_keys = c.take<unsigned long long>((size_t)n_seg * cap);
        }))) return rc;
    Trim2Args a{};
    a.in = in;
    a.out = out;
    a.order = d_ord;
    a.n_rules = n_rules;
    for (uint32_t r = 0; r < n_rules; ++r) {
        a.r_count[r] = rules[r].count;
        a.r_source[r] = rules[r].source;
        a.r_type[r] = rules[r].type;
    }
    if ((rc = uniform_offsets_locked(ctx, n_seg, cap, d_off))) return rc;
    trim2_keys_kernel<<<dim3((cap + 255) / 256, n_rules, nq), 256, 0, ctx->stream>>>(a, d_keys);
    PG_HIP(hipGetLastError());
    // (what the sort makes of padding and of non-members does not matter: the cut skips them wherever they lie in the order)
    if ((rc = sort_dev_locked(ctx, reinterpret_cast<const double*>(d_keys), d_off, n_seg, n_seg * cap, cap, 1, d_ord))) return rc;
    candidates_trim2_kernel<<<nq, kTrim2Chunk, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_trim2_out_cap(const pg_trim_rule* rules, uint32_t n_rules, uint32_t cap, uint32_t* out_cap) {
    PG_REQUIRE(out_cap, "pg_trim2_out_cap: NULL argument");
    return pg::trim2_check_rules(rules, n_rules, cap, out_cap, "pg_trim2_out_cap");
}

int pg_candidates_trim2_dev(pg_ctx* ctx, const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                            const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                            uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                            double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                            float* d_out_planes_f32, uint32_t* d_out_count) {
    PG_REQUIRE(ctx, "pg_candidates_trim2_dev: NULL argument");
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    uint32_t out_cap = 0;
    int rc;
    if ((rc = pg::trim2_check_call(rules, n_rules, nq, cap, l, &out_cap, "pg_candidates_trim2_dev"))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::candidates_trim2_locked(ctx, rules, n_rules, in, out);
}

int pg_candidates_trim2_host(const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const uint64_t* rows,
                             const double* score, const uint8_t* source, const uint32_t* count, const double* planes_f64, uint32_t n_f64,
                             const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32, uint64_t* out_rows, double* out_score,
                             uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32,
                             uint32_t* out_count) {
    const pg::CandCall l{rows, score, source, count, planes_f64, n_f64, source_mask, planes_f32, n_f32, out_rows, out_score,
                         out_source, out_planes_f64, out_source_mask, out_planes_f32, out_count};
    uint32_t out_cap = 0;
    int rc;
    if ((rc = pg::trim2_check_call(rules, n_rules, nq, cap, l, &out_cap, "pg_candidates_trim2_host"))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    std::vector<uint32_t> list;
    std::vector<double> key(cap);
    std::vector<bool> via_plane(cap), taken(cap);
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
        const uint32_t n_valid = pg::cand_n_valid(in, q);
        std::fill(taken.begin(), taken.end(), false);
        uint64_t acc = 0;
        uint32_t n = 0;
        for (uint32_t c = 0; c < n_rules; ++c) {
            const uint32_t sc = rules[c].source;
            list.clear();
            for (uint32_t p = 0; p < cap; ++p) {                  // (:58,63,66-71)
                bool plane;
                if (!pg::trim2_member(in, in0 + p, p, n_valid, sc, &plane)) continue;
                key[p] = pg::cand_bits_f64(pg::trim2_key(in, in0 + p, sc, plane));
                via_plane[p] = plane;
                list.push_back(p);
            }
            std::stable_sort(list.begin(), list.end(), [&](uint32_t x, uint32_t y) { return pg::cand_before(key[x], key[y]); });    // (:74)
            const uint64_t cnt = rules[c].count;
            const uint64_t limit = rules[c].type == PG_TRIM_FIX ? cnt : (cnt > acc ? cnt - acc : 0);     // (:76-77,86-88)
            uint64_t picks = 0;
            for (size_t j = 0; j < list.size() && picks < limit; ++j) {
                const uint32_t p = list[j];
                if (taken[p]) continue;                           // (deleted from the map by the rule that took it, :80-83,91-93)
                taken[p] = true;
                ++picks;
                if (n >= out_cap) continue;                       // (never: pg_trim2_out_cap's bound)
                const size_t src = in0 + p, o = out0 + n++;
                pg::cand_carry(in, out, src, o, false);
                out.score[o] = pg::trim2_key(in, src, sc, via_plane[p]);
                if (out.source) out.source[o] = (uint8_t)sc;
            }
            if (rules[c].type != PG_TRIM_FIX) acc += picks;       // (:95)
        }
        pg::cand_pad(in, out, q, n, 1, pg::kCandNegInf);
        out_count[q] = n;
    }
    return PG_OK;
}

}  // extern "C"
