// blend.hip — a request's merged candidates interleaved by recall on the device: SnakeFilter and CompletelyFairCountFilter
// (DESIGN.md 4.1q).
//
// Both sit in the trim's slot between UniqueFilter and RankService.Rank (service/user_recommend.go:105-137).  SnakeFilter
// (filter/snake_filter.go:173-241) orders every configured recall by its own score — an item that several recalls hold stands in
// each of their lists, keyed by that recall's score (RecallScores) — and deals the lists out round after round by weight;
// CompletelyFairCountFilter (filter/completely_fair_count_filter.go:34-94) sorts the merged list by score and deals the recalls
// out one item at a time.  The orders are the score sort's (sort.hip); the kernels here turn them into the output permutation
// and gather every carried array through it: one workgroup per request, no value meets arithmetic.
//   FAIR    count   real entries and first appearance in the order, per source (wave ballots added up in LDS);
//           plan    one lane: between two exhaustions the slot table is constant, so at most 8 phases, each {first count, stride
//                   = names left} per source;
//           walk    the sorted order in chunks as trim.hip's walk: an entry's rank within its source → its phase → its output
//                   position; no loop over retain;
//   SNAKE   keys    one key array per config entry (members: the score or the recall's plane; everything else NaN), sorted as
//                   nq x n_entries segments;
//           compact each entry's order to its members, in order (block_rank.hpp's chunk_rank): the sort cannot tell a
//                   non-member from a member with a NaN key; the head of every list is kept in LDS as uint16;
//           walk    one wave, a (round, entry) step at a time, 64 list entries per look: ballot the untaken ones against a bitmap
//                   of input positions in LDS, take by wave_rank, mark, record {position, entry} at the running output position;
//           gather  the whole workgroup, from the pick records;
//   pad     the slots behind the kept entries.
// pg_candidates_blend_host states the same answer on host arrays with plain containers; the tests hold the device to it.
#include "pipeline.hpp"
#include "block_rank.hpp"

#include <algorithm>
#include <vector>

namespace pg {
namespace {

constexpr uint32_t kBlendMaxSources = 8;
constexpr uint32_t kBlendMaxPlanes = 8;
constexpr uint32_t kBlendMaxCap = 16384;
static_assert(kBlendMaxSources == PG_BLEND_MAX_SOURCES && kBlendMaxPlanes == PG_BLEND_MAX_PLANES && kBlendMaxCap == PG_BLEND_MAX_CAP,
              "include/pairec_gpu.h repeats these");
static_assert(kBlendMaxSources == kCandMaxSources && kBlendMaxPlanes == kCandMaxPlanes && kBlendMaxCap == kCandMaxCap,
              "the header names the limits per stage; cand_lists.hpp holds them together");
constexpr uint32_t kBlendThreads = 1024;         // positions walked at a time
constexpr uint32_t kBlendWaves = kBlendThreads / kWave;
constexpr uint32_t kBlendLdsList = 2064;         // entries of every compacted list kept in LDS (uint16 positions): 8 x 2064 x 2 B = 33 KB
constexpr uint32_t kBlendNone = 0xFFu;           // the source of padding
static_assert(kBlendMaxCap <= 65536 && kBlendMaxCap % 32 == 0, "positions fit uint16 and the pick records' low half; the bitmap is whole words");

struct BlendArgs {
    CandIn in;                                   // (source NULL: every real entry belongs to one source)
    CandOut out;
    const uint32_t* order;                       // FAIR [nq][cap], SNAKE [nq][n_entries][cap]: positions in score order
    uint32_t* lists;                             // SNAKE [nq][n_entries][cap]: every entry's members in order
    uint32_t* picks;                             // SNAKE [nq][out_cap]: position | entry << 16, in pick order
    uint32_t skip, retain, n_entries;
    uint32_t e_weight[kBlendMaxSources];
    uint8_t e_source[kBlendMaxSources];
};

// the source of the entry at position p of the request, kBlendNone for padding
__device__ inline uint32_t blend_source(const BlendArgs& a, size_t in0, uint32_t p, uint32_t n_valid) {
    if (p >= n_valid || a.in.rows[in0 + p] == kCandPad) return kBlendNone;
    if (!a.in.source) return a.e_source[0];      // (FAIR: 0)
    const uint32_t s = a.in.source[in0 + p];
    return s < kBlendMaxSources ? s : kBlendNone;
}

// SNAKE: does the real entry at p, of source s, stand in the list of the entry that names source si — and with which key
// (snake_filter.go:63-67,188-200)
__device__ inline bool blend_member(const BlendArgs& a, size_t in0, uint32_t p, uint32_t s, uint32_t si, bool* own) {
    *own = s == si;
    if (s == si) return true;
    if (!a.in.mask) return false;
    const uint32_t m = a.in.mask[in0 + p];
    return __popc(m) > 1 && ((m >> si) & 1u);
}

// SNAKE keys: key[q][i][p] = the key of position p in entry i's list, NaN where it is no member (it sorts behind every number; the
// walk kernel drops it again)
__global__ __launch_bounds__(256) void blend_keys_kernel(BlendArgs a, unsigned long long* keys) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x, i = blockIdx.y, q = blockIdx.z;
    const uint32_t cap = a.in.cap;
    if (p >= cap) return;
    const size_t in0 = (size_t)q * cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    const uint32_t s = blend_source(a, in0, p, n_valid), si = a.e_source[i];
    unsigned long long k = kCandNan;
    bool own;
    if (s != kBlendNone && blend_member(a, in0, p, s, si, &own))
        k = own ? a.in.score[in0 + p] : a.in.planes64[(size_t)si * a.in.nq * cap + in0 + p];
    keys[((size_t)q * a.n_entries + i) * cap + p] = k;
}

// SNAKE, request q = blockIdx.x.
__global__ __launch_bounds__(kBlendThreads) void blend_snake_kernel(BlendArgs a) {
    __shared__ uint16_t head[kBlendMaxSources][kBlendLdsList];
    __shared__ uint32_t taken[kBlendMaxCap / 32];
    __shared__ uint32_t llen[kBlendMaxSources], cur[kBlendMaxSources];
    __shared__ uint32_t wcnt[2 * kBlendWaves];
    __shared__ uint32_t total_s;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t cap = a.in.cap, out_cap = a.out.out_cap, n_e = a.n_entries;
    const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    for (uint32_t w = tid; w < kBlendMaxCap / 32; w += kBlendThreads) taken[w] = 0u;
    if (tid < kBlendMaxSources) {
        llen[tid] = 0;
        cur[tid] = 0;
    }
    __syncthreads();
    // compact: every entry's order → its members, in order
    uint32_t it = 0;
    for (uint32_t i = 0; i < n_e; ++i) {
        const size_t l0 = ((size_t)q * n_e + i) * cap;
        const uint32_t si = a.e_source[i];
        for (uint32_t c0 = 0; c0 < cap; c0 += kBlendThreads, ++it) {
            const uint32_t j = c0 + tid;
            uint32_t pos = 0;
            bool mem = false;
            if (j < cap) {
                pos = a.order[l0 + j];
                if (pos < cap) {
                    const uint32_t s = blend_source(a, in0, pos, n_valid);
                    bool own;
                    mem = s != kBlendNone && blend_member(a, in0, pos, s, si, &own);
                }
            }
            uint32_t r, total;
            chunk_rank<kBlendWaves>(mem, wcnt, it, &r, &total);
            if (mem) {
                const uint32_t rank = llen[i] + r;
                a.lists[l0 + rank] = pos;                        // (rank < cap: ranks count distinct positions of the order)
                if (rank < kBlendLdsList) head[i][rank] = (uint16_t)pos;
            }
            __syncthreads();
            // (the length moves between this chunk's reads and the next chunk's, which lie behind its barrier)
            if (tid == 0) llen[i] += total;
        }
    }
    __syncthreads();
    // walk (snake_filter.go:212-231; Next :76-109): one wave, every quantity that steers it is the same in all its lanes.
    // One wave alone waits for its instruction fetches: where the loops below fall in the 64-byte instruction lines moves REFILL
    // and SKIP by 1 to 1.5 % each (profiles/cand_lists_refactor.json, "placement"), so the walk starts at a fixed place in a line,
    // the one of three measured at which both run as they did before the lists moved to cand_lists.hpp, whatever the code before
    // it comes to.
    asm volatile(".p2align 6\n\ts_nop 0");
    if (wave == 0) {
        const uint32_t retain = a.retain;
        uint32_t size = 0, outp = 0;
        while (size < retain) {
            uint32_t round = 0;
            for (uint32_t i = 0; i < n_e; ++i) {
                const size_t l0 = ((size_t)q * n_e + i) * cap;
                const uint32_t len = llen[i];
                uint32_t w = a.e_weight[i], c = cur[i];
                while (w > 0 && c < len) {
                    uint32_t n = min((uint32_t)kWave, len - c);
                    if (a.skip) n = min(n, w);                   // SKIP: every entry looked at costs a slot
                    const bool have = lane < n;
                    uint32_t pos = 0;
                    if (have) pos = c + lane < kBlendLdsList ? (uint32_t)head[i][c + lane] : a.lists[l0 + c + lane];
                    const bool fresh = have && !((taken[pos >> 5] >> (pos & 31u)) & 1u);
                    uint32_t nf;
                    const uint32_t before = wave_rank(fresh, &nf);
                    uint32_t used = n, np = nf;
                    bool take = fresh;
                    if (a.skip) {
                        w -= n;
                    } else {
                        if (nf >= w) {                           // REFILL: the w-th fresh entry ends the step, the cursor stands behind it
                            const unsigned long long last = __ballot(fresh && before == w - 1);
                            used = (uint32_t)__builtin_ctzll(last) + 1u;
                            take = fresh && before < w;
                            np = w;
                        }
                        w -= np;
                    }
                    if (take) {
                        atomicOr(&taken[pos >> 5], 1u << (pos & 31u));
                        const uint32_t o = outp + before;
                        if (o < out_cap) a.picks[out0 + o] = pos | (i << 16);      // (picks past retain_num are cut, :229-231)
                    }
                    outp += np;
                    round += np;
                    c += used;
                    // the marks of this look are in LDS before the next look reads the bitmap
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                }
                cur[i] = c;                                      // (every lane writes the value every lane reads back)
            }
            if (round == 0) break;                               // (:223-225)
            size += round;
        }
        if (lane == 0) total_s = min(outp, out_cap);             // (out_cap = min(cap, retain_num), picks <= real entries <= cap)
    }
    __syncthreads();
    // gather: a pick carries its key in the picking list and that list's source (:83-88)
    const uint32_t total = total_s;
    for (uint32_t j = tid; j < total; j += kBlendThreads) {
        const uint32_t rec = a.picks[out0 + j], pos = rec & 0xFFFFu, i = rec >> 16;
        const uint32_t si = a.e_source[i];
        const size_t src = in0 + pos, o = out0 + j;
        const bool own = !a.in.source || a.in.source[src] == si;
        cand_carry(a.in, a.out, src, o, false);
        a.out.score[o] = own ? a.in.score[src] : a.in.planes64[(size_t)si * a.in.nq * cap + src];
        if (a.out.source) a.out.source[o] = (uint8_t)si;
    }
    cand_pad(a.in, a.out, q, total + tid, kBlendThreads, kCandNegInf);
    if (tid == 0) a.out.count[q] = total;
}

// FAIR, request q = blockIdx.x.
__global__ __launch_bounds__(kBlendThreads) void blend_fair_kernel(BlendArgs a) {
    __shared__ uint32_t cnt[kBlendMaxSources], first[kBlendMaxSources], run[kBlendMaxSources];
    __shared__ uint32_t wcnt[2][kBlendMaxSources][kBlendWaves];
    // the plan: in phase p source s gives ph_g entries, its ph_r0-th onwards, at counts ph_first, ph_first + ph_k, ...
    __shared__ uint32_t ph_first[kBlendMaxSources][kBlendMaxSources], ph_r0[kBlendMaxSources][kBlendMaxSources],
        ph_g[kBlendMaxSources][kBlendMaxSources], ph_k[kBlendMaxSources];
    __shared__ uint32_t n_ph_s, total_s;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t cap = a.in.cap, out_cap = a.out.out_cap;
    const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    if (tid < kBlendMaxSources) {
        cnt[tid] = 0;
        run[tid] = 0;
        first[tid] = 0xFFFFFFFFu;
    }
    __syncthreads();
    // count: every source's real entries and where it first appears in the order (completely_fair_count_filter.go:59-65)
    for (uint32_t c0 = 0; c0 < cap; c0 += kBlendThreads) {
        const uint32_t i = c0 + tid;
        uint32_t s = kBlendNone;
        if (i < cap) {
            const uint32_t pos = a.order[in0 + i];
            if (pos < cap) s = blend_source(a, in0, pos, n_valid);
        }
        for (uint32_t r = 0; r < kBlendMaxSources; ++r) {
            const unsigned long long m = __ballot(s == r);
            if (lane == 0 && m) {
                atomicAdd(&cnt[r], (uint32_t)__popcll(m));
                atomicMin(&first[r], c0 + wave * kWave + (uint32_t)__builtin_ctzll(m));
            }
        }
    }
    __syncthreads();
    // plan (:72-89): between two exhaustions the slot table is constant — slot i of k, in a phase that starts at count c0,
    // gives at c0 + ((i - c0) mod k) and every k counts after; the slot that gives its last entry first ends the phase
    if (tid == 0) {
        uint32_t names[kBlendMaxSources], rem[kBlendMaxSources], given[kBlendMaxSources], fi[kBlendMaxSources];
        uint32_t k = 0, real = 0;
        for (uint32_t s = 0; s < kBlendMaxSources; ++s) {
            rem[s] = cnt[s];
            given[s] = 0;
            real += cnt[s];
            if (cnt[s]) {                                        // names in order of first appearance
                uint32_t at = k++;
                while (at > 0 && first[names[at - 1]] > first[s]) {
                    names[at] = names[at - 1];
                    --at;
                }
                names[at] = s;
            }
        }
        const uint32_t retain = min(a.retain, real);
        uint32_t c0 = 0, np = 0;
        while (c0 < retain && k > 0 && np < kBlendMaxSources) {
            uint32_t e_star = 0xFFFFFFFFu, i_star = 0;
            for (uint32_t i = 0; i < k; ++i) {
                const uint32_t f = c0 + (i + k - c0 % k) % k, ex = f + (rem[names[i]] - 1u) * k;
                fi[i] = f;
                if (ex < e_star) {
                    e_star = ex;
                    i_star = i;
                }
            }
            const uint32_t c_end = min(e_star, retain - 1u);
            for (uint32_t s = 0; s < kBlendMaxSources; ++s) ph_g[np][s] = 0;
            for (uint32_t i = 0; i < k; ++i) {
                const uint32_t s = names[i], g = fi[i] <= c_end ? (c_end - fi[i]) / k + 1u : 0u;
                ph_first[np][s] = fi[i];
                ph_r0[np][s] = given[s];
                ph_g[np][s] = g;
                given[s] += g;
                rem[s] -= g;
            }
            ph_k[np] = k;
            ++np;
            c0 = c_end + 1u;
            if (c_end == e_star) {                               // (:80-83)
                names[i_star] = names[k - 1];
                --k;
            }
        }
        n_ph_s = np;
        total_s = min(retain, out_cap);
    }
    __syncthreads();
    const uint32_t n_ph = n_ph_s;
    // walk: the sorted order, chunk after chunk
    for (uint32_t c0 = 0, it = 0; c0 < cap; c0 += kBlendThreads, ++it) {
        const uint32_t i = c0 + tid;
        uint32_t pos = 0, s = kBlendNone;
        if (i < cap) {
            pos = a.order[in0 + i];
            if (pos < cap) s = blend_source(a, in0, pos, n_valid);
        }
        uint32_t(*wc)[kBlendWaves] = wcnt[it & 1u];          // (two sets of counts: a wave ahead by one chunk writes the other one)
        uint32_t before = 0;
        for (uint32_t r = 0; r < kBlendMaxSources; ++r) {
            const unsigned long long m = __ballot(s == r);
            if (s == r) before = ballot_rank(m);
            if (lane == 0) wc[r][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (s != kBlendNone) {
            uint32_t rank = run[s] + before;
            for (uint32_t w = 0; w < wave; ++w) rank += wc[s][w];
            uint32_t dst = 0xFFFFFFFFu;
            for (uint32_t p = 0; p < n_ph; ++p)
                if (rank >= ph_r0[p][s] && rank - ph_r0[p][s] < ph_g[p][s]) dst = ph_first[p][s] + (rank - ph_r0[p][s]) * ph_k[p];
            if (dst < out_cap) {
                const size_t src = in0 + pos, o = out0 + dst;
                cand_carry(a.in, a.out, src, o, false);
                a.out.score[o] = a.in.score[src];
                if (a.out.source) a.out.source[o] = a.in.source[src];
            }
        }
        __syncthreads();
        // (the running counts move between this chunk's reads and the next chunk's, which lie behind its barrier)
        if (tid < kBlendMaxSources) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < kBlendWaves; ++w) t += wc[tid][w];
            run[tid] += t;
        }
    }
    const uint32_t total = total_s;
    cand_pad(a.in, a.out, q, total + tid, kBlendThreads, kCandNegInf);
    if (tid == 0) a.out.count[q] = total;
}

// the conf as the reference can run it, and the width of what it keeps
int blend_check_conf(const pg_blend_conf* c, uint32_t cap, uint32_t* out_cap, const char* who) {
    if (!c) {
        set_error("%s: NULL conf", who);
        return PG_ERR_INVALID;
    }
    if (c->mode != PG_BLEND_SNAKE_REFILL && c->mode != PG_BLEND_SNAKE_SKIP && c->mode != PG_BLEND_FAIR) {
        set_error("%s: mode %u (PG_BLEND_SNAKE_REFILL, PG_BLEND_SNAKE_SKIP or PG_BLEND_FAIR)", who, c->mode);
        return PG_ERR_INVALID;
    }
    if (c->retain_num == 0) {
        set_error("%s: retain_num is 0 (nothing would be kept)", who);
        return PG_ERR_INVALID;
    }
    if (c->mode != PG_BLEND_FAIR) {
        if (c->n_entries > kBlendMaxSources) {
            set_error("%s: n_entries=%u unsupported (1..%u)", who, c->n_entries, kBlendMaxSources);
            return PG_ERR_UNSUPPORTED;
        }
        if (c->n_entries == 0) {
            set_error("%s: a snake without entries (AdjustCountConfs is empty)", who);
            return PG_ERR_INVALID;
        }
        uint32_t seen = 0;
        bool any_weight = false;
        for (uint32_t i = 0; i < c->n_entries; ++i) {
            if (c->source[i] >= kBlendMaxSources) {
                set_error("%s: entry %u names source %u (< %u)", who, i, c->source[i], kBlendMaxSources);
                return PG_ERR_INVALID;
            }
            if ((seen >> c->source[i]) & 1u) {
                set_error("%s: source %u is named twice (the reference's map keeps only the later iterator)", who, c->source[i]);
                return PG_ERR_INVALID;
            }
            seen |= 1u << c->source[i];
            any_weight = any_weight || c->weight[i] != 0;
        }
        if (!any_weight) {
            set_error("%s: every weight is 0 (the reference divides 0 by 0 for its counts)", who);
            return PG_ERR_INVALID;
        }
    }
    if (cap < 1 || cap > kBlendMaxCap) {
        set_error("%s: cap=%u unsupported (1..%u)", who, cap, kBlendMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    if (out_cap) *out_cap = std::min(cap, c->retain_num);
    return PG_OK;
}

// the checks both entry points share, in the order they fire: the pointers, nq, the conf, the pairs of optional arrays, what a
// snake needs of them (an output may share memory with its input: the blend does not ask)
int blend_check_call(const pg_blend_conf* c, uint32_t nq, uint32_t cap, const CandCall& l, uint32_t* out_cap, const char* who) {
    int rc;
    if ((rc = cand_call_required(l, true, who)) || (rc = cand_check_nq(nq, who)) || (rc = blend_check_conf(c, cap, out_cap, who)) ||
        (rc = cand_lists_check(l, kBlendMaxPlanes, who)))
        return rc;
    if (c->mode != PG_BLEND_FAIR) {
        PG_REQUIRE(l.source || c->n_entries == 1, "%s: a snake that names more than one source needs d_source", who);
        if (l.source_mask) {
            uint32_t need = 0;
            for (uint32_t i = 0; i < c->n_entries; ++i) need = std::max(need, (uint32_t)c->source[i] + 1u);
            PG_REQUIRE(l.planes_f64 && l.n_f64 >= need,
                       "%s: a source mask needs the per-recall score planes of every named source (n_f64 >= %u)", who, need);
        }
    }
    return PG_OK;
}

// one request of pg_candidates_blend_host → the input positions kept, with the entry (SNAKE) each was picked through
struct BlendPick {
    uint32_t pos, entry;
};
void blend_request_host(const pg_blend_conf& c, uint32_t cap, const uint64_t* rows, const double* score, const uint8_t* source,
                        uint32_t n_valid, const double* planes_f64, size_t plane_stride, const uint32_t* mask, std::vector<BlendPick>* out) {
    out->clear();
    auto src_of = [&](uint32_t p) -> uint32_t {
        if (p >= n_valid || rows[p] == ~0ull) return kBlendNone;
        if (!source) return c.mode == PG_BLEND_FAIR ? 0u : c.source[0];
        return source[p] < kBlendMaxSources ? source[p] : kBlendNone;
    };
    if (c.mode == PG_BLEND_FAIR) {
        std::vector<uint32_t> real;
        for (uint32_t p = 0; p < cap; ++p)
            if (src_of(p) != kBlendNone) real.push_back(p);
        const size_t retain = std::min<size_t>(c.retain_num, real.size());
        std::stable_sort(real.begin(), real.end(), [&](uint32_t x, uint32_t y) { return cand_before(score[x], score[y]); });
        std::vector<uint32_t> by[kBlendMaxSources];
        size_t at[kBlendMaxSources] = {0};
        std::vector<uint32_t> names;
        for (uint32_t p : real) {                                 // (:59-65)
            const uint32_t s = src_of(p);
            if (by[s].empty()) names.push_back(s);
            by[s].push_back(p);
        }
        size_t count = 0;
        while (count < retain) {                                  // (:72-89)
            const size_t i = count % names.size();
            const uint32_t s = names[i];
            out->push_back({by[s][at[s]++], 0u});
            ++count;
            if (at[s] == by[s].size()) {
                names[i] = names.back();
                names.pop_back();
            }
        }
        return;
    }
    std::vector<uint32_t> lists[kBlendMaxSources];
    for (uint32_t i = 0; i < c.n_entries; ++i) {
        const uint32_t si = c.source[i];
        std::vector<double> key(cap, 0.0);
        for (uint32_t p = 0; p < cap; ++p) {
            const uint32_t s = src_of(p);
            if (s == kBlendNone) continue;
            if (s == si) {
                key[p] = score[p];
                lists[i].push_back(p);
            } else if (mask && __builtin_popcount(mask[p]) > 1 && ((mask[p] >> si) & 1u)) {
                key[p] = planes_f64[si * plane_stride + p];
                lists[i].push_back(p);
            }
        }
        std::stable_sort(lists[i].begin(), lists[i].end(), [&](uint32_t x, uint32_t y) { return cand_before(key[x], key[y]); });
    }
    std::vector<bool> taken(cap, false);
    size_t cur[kBlendMaxSources] = {0};
    const bool skip = c.mode == PG_BLEND_SNAKE_SKIP;
    size_t size = 0;
    while (size < c.retain_num) {                                 // (:212-227)
        size_t round = 0;
        for (uint32_t i = 0; i < c.n_entries; ++i) {
            uint32_t slots = 0;
            while (slots < c.weight[i] && cur[i] < lists[i].size()) {     // (Next, :76-109)
                const uint32_t p = lists[i][cur[i]++];
                if (!taken[p]) {
                    taken[p] = true;
                    out->push_back({p, i});
                    ++slots;
                    ++round;
                } else if (skip) {
                    ++slots;
                }
            }
        }
        if (round == 0) break;
        size += round;
    }
    if (out->size() > c.retain_num) out->resize(c.retain_num);    // (:229-231)
}

}  // namespace

int candidates_blend_locked(pg_ctx* ctx, const pg_blend_conf* conf, const CandIn& in, const CandOut& out) {
    const uint32_t nq = in.nq, cap = in.cap;
    int rc;
    const bool fair = conf->mode == PG_BLEND_FAIR;
    const uint32_t n_e = fair ? 1u : conf->n_entries, n_seg = nq * n_e;
    // scratch: segment offsets | orders | (SNAKE) keys | lists | pick records
    uint32_t *d_off, *d_ord, *d_lists, *d_picks; unsigned long long* d_keys;
    if ((rc = scratch_carve(ctx, kSlotBlend, [&](Carve& c) {
            d_off = c.take<uint32_t>((size_t)n_seg + 1);
            d_ord = c.take<uint32_t>((size_t)n_seg * cap);
            d_keys = c.take<unsigned long long>(fair ? 0 : (size_t)n_seg * cap);
            d_lists = c.take<uint32_t>(fair ? 0 : (size_t)n_seg * cap);
            d_picks = c.take<uint32_t>(fair ? 0 : (size_t)nq * out.out_cap);
        }))) return rc;
    BlendArgs a{};
    a.in = in;
    a.out = out;
    a.order = d_ord;
    a.lists = fair ? nullptr : d_lists;
    a.picks = fair ? nullptr : d_picks;
    a.skip = conf->mode == PG_BLEND_SNAKE_SKIP ? 1u : 0u;
    a.retain = conf->retain_num;
    a.n_entries = n_e;
    for (uint32_t i = 0; i < kBlendMaxSources; ++i) {
        a.e_weight[i] = !fair && i < n_e ? conf->weight[i] : 0u;
        a.e_source[i] = !fair && i < n_e ? conf->source[i] : 0u;
    }
    if ((rc = uniform_offsets_locked(ctx, n_seg, cap, d_off))) return rc;
    // (what the sorts make of padding and of non-members does not matter: the kernels skip them wherever they lie in the order)
    if (fair) {
        if ((rc = sort_dev_locked(ctx, reinterpret_cast<const double*>(in.score), d_off, n_seg, n_seg * cap, cap, 1, d_ord))) return rc;
        blend_fair_kernel<<<nq, kBlendThreads, 0, ctx->stream>>>(a);
    } else {
        blend_keys_kernel<<<dim3((cap + 255) / 256, n_e, nq), 256, 0, ctx->stream>>>(a, d_keys);
        PG_HIP(hipGetLastError());
        if ((rc = sort_dev_locked(ctx, reinterpret_cast<const double*>(d_keys), d_off, n_seg, n_seg * cap, cap, 1, d_ord))) return rc;
        blend_snake_kernel<<<nq, kBlendThreads, 0, ctx->stream>>>(a);
    }
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_blend_out_cap(const pg_blend_conf* conf, uint32_t cap, uint32_t* out_cap) {
    PG_REQUIRE(out_cap, "pg_blend_out_cap: NULL argument");
    return pg::blend_check_conf(conf, cap, out_cap, "pg_blend_out_cap");
}

int pg_candidates_blend_dev(pg_ctx* ctx, const pg_blend_conf* conf, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                            const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                            uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                            double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                            float* d_out_planes_f32, uint32_t* d_out_count) {
    PG_REQUIRE(ctx, "pg_candidates_blend_dev: NULL argument");
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    uint32_t out_cap = 0;
    int rc;
    if ((rc = pg::blend_check_call(conf, nq, cap, l, &out_cap, "pg_candidates_blend_dev"))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::candidates_blend_locked(ctx, conf, in, out);
}

int pg_candidates_blend_host(const pg_blend_conf* conf, uint32_t nq, uint32_t cap, const uint64_t* rows, const double* score,
                             const uint8_t* source, const uint32_t* count, const double* planes_f64, uint32_t n_f64,
                             const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32, uint64_t* out_rows, double* out_score,
                             uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32,
                             uint32_t* out_count) {
    const pg::CandCall l{rows, score, source, count, planes_f64, n_f64, source_mask, planes_f32, n_f32, out_rows, out_score,
                         out_source, out_planes_f64, out_source_mask, out_planes_f32, out_count};
    uint32_t out_cap = 0;
    int rc;
    if ((rc = pg::blend_check_call(conf, nq, cap, l, &out_cap, "pg_candidates_blend_host"))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    std::vector<pg::BlendPick> picks;
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
        pg::blend_request_host(*conf, cap, rows + in0, score + in0, source ? source + in0 : nullptr, pg::cand_n_valid(in, q),
                               planes_f64 ? planes_f64 + in0 : nullptr, (size_t)nq * cap, source_mask ? source_mask + in0 : nullptr, &picks);
        const uint32_t n = (uint32_t)std::min<size_t>(picks.size(), out_cap);
        for (uint32_t j = 0; j < n; ++j) {
            const size_t src = in0 + picks[j].pos, o = out0 + j;
            pg::cand_carry(in, out, src, o, conf->mode == PG_BLEND_FAIR);
            if (conf->mode != PG_BLEND_FAIR) {
                const uint32_t si = conf->source[picks[j].entry];
                const bool own = !source || source[src] == si;
                out.score[o] = own ? in.score[src] : in.planes64[si * ((size_t)nq * cap) + src];
                if (out.source) out.source[o] = (uint8_t)si;
            }
        }
        pg::cand_pad(in, out, q, n, 1, pg::kCandNegInf);
        out_count[q] = n;
    }
    return PG_OK;
}

}  // extern "C"
