// diversity.hip — DiversityRuleSort on the device: windowed scatter rules per request.
//
// The re-rank that follows ItemRankScore in most scenes (sort/diversity_rule_sort.go:116-283): a greedy loop that appends, step
// by step, the first remaining candidate that no rule rejects against the tail of the result — at most `frequency` entries of a
// value in any `window`, never `interval` in a row (sort/diversity_rule.go:50-92) — keeps some entries off some positions
// (sort/diversity_exclusion_rule.go:37-56) and falls back to the candidate with the heaviest set of satisfied rules.  The answer
// is defined bit for bit in include/pairec_gpu.h; div_host_one below states it on the host, the kernel reproduces it.
//
// One workgroup per request, every decision taken by all lanes alike from what lies in LDS:
//   compact  the entries that are not set aside, in order (block_rank.hpp's wave_rank + per-wave counts of both flags behind
//            one barrier); the set-aside ones behind them, reversed;
//   keys     per rule, an entry's value becomes the smallest position that holds an equal tuple: an open-addressed table in the
//            request's slice of context scratch whose slots hold positions — two entries share a slot iff their TUPLES are equal,
//            compared column by column; every access of a slot is an agent-scope atomic (fanin.hip's scratch tier);
//   bits     one bit per (exclusion rule, entry): its terms evaluated once;
//   greedy   per step: scan kDivChunk entries at a time from the first untaken one; a lane tests its entry against every rule
//            with two reads per rule — the run of equal values at the result's tail (interval) and the count of its value among the
//            last window - 1 results (window), both kept current by one lane per rule after every pick; ballots + a scan of the
//            waves' masks give the first eligible entry (which fixes the explore bound) and the first passing one; (largest w,
//            first position) travels packed in one 64-bit maximum;
//   output   the result, the untaken entries in order (block_rank.hpp's chunk_rank), the set-aside entries, UINT32_MAX behind count.
// The window counts and the keys live in context scratch, written by one lane and read by the workgroup's others only across
// a __syncthreads: one workgroup stays on one compute unit, whose vector cache serves them all.
#include "cand_lists.hpp"
#include "block_rank.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <thread>
#include <vector>

namespace pg {
namespace {

constexpr uint32_t kDivMaxN = 8192;
constexpr uint32_t kDivMaxRules = 8;
constexpr uint32_t kDivMaxDims = 4;
constexpr uint32_t kDivMaxCols = 16;
constexpr uint32_t kDivMaxExcl = 8;
constexpr uint32_t kDivMaxTerms = 4;
constexpr uint32_t kDivMaxPositions = 64;
constexpr uint32_t kDivChunk = 1024;             // entries scanned at a time = the workgroup's lanes
static_assert(kDivMaxN == PG_DIV_MAX_N && kDivMaxRules == PG_DIV_MAX_RULES && kDivMaxDims == PG_DIV_MAX_DIMS &&
                  kDivMaxCols == PG_DIV_MAX_COLS && kDivMaxExcl == PG_DIV_MAX_EXCL && kDivMaxTerms == PG_DIV_MAX_TERMS &&
                  kDivMaxPositions == PG_DIV_MAX_POSITIONS && kDivChunk == PG_DIV_CHUNK,
              "include/pairec_gpu.h repeats these");
constexpr uint32_t kDivThreads = kDivChunk;
constexpr uint32_t kDivWaves = kDivThreads / kWave;
constexpr uint32_t kDivMinSlots = 1024;          // slots = the power of two >= max(2 cap, this): load factor <= 0.5
constexpr uint32_t kDivNone = 0xFFFFFFFFu;
static_assert(kDivMaxN <= 0xFFFFu, "positions travel as uint16 in LDS and in the packed (w, position)");
static_assert(kDivWaves <= 64, "one lane per wave mask");

// the validated config as the kernel and the host function read it
struct DivRule {
    uint32_t n_dims, dims[kDivMaxDims];
    int32_t interval, window, frequency, weight;
    uint32_t win_on;                             // window > 0 && frequency > 0 && window > frequency
};
struct DivTerm {
    uint32_t column;
    int32_t op;
    long long value;
};
struct DivExcl {
    uint32_t n_pos, n_terms;
    uint16_t pos[kDivMaxPositions];              // ascending, distinct, <= kDivMaxN + 1
    DivTerm terms[kDivMaxTerms];
};
struct DivCfg {
    int32_t size, diversity_size, explore;
    uint32_t exclude_mask, n_cols, n_rules, n_excl, has_weight;
    DivRule rules[kDivMaxRules];
    DivExcl excl[kDivMaxExcl];
};

struct DivArgs {
    DivCfg c;
    const long long* dims;                       // [n_cols][nq][cap]
    const uint8_t* source;                       // [nq][cap] or NULL
    const uint32_t* count;                       // [nq] or NULL
    const uint8_t* enable;                       // [nq] or NULL
    uint32_t* order;                             // [nq][cap]
    uint32_t* keys;                              // scratch [nq][n_rules][cap]
    uint32_t* cnt;                               // scratch [nq][n_rules][cap]
    uint32_t* tbl;                               // scratch [nq][1 << slot_bits]
    uint32_t nq, cap, slot_bits;
};
static_assert(sizeof(DivArgs) <= 3072, "kernel arguments");

__host__ __device__ inline bool div_term_holds(int32_t op, long long v, long long c) {
    switch (op) {
        case PG_WHERE_GT: return v > c;
        case PG_WHERE_GE: return v >= c;
        case PG_WHERE_LT: return v < c;
        case PG_WHERE_LE: return v <= c;
        case PG_WHERE_EQ: return v == c;
        default: return v != c;
    }
}

__device__ inline bool div_tuple_eq(const long long* d, size_t plane, const DivRule& r, uint32_t pa, uint32_t pb) {
    bool eq = true;
    for (uint32_t k = 0; k < r.n_dims; ++k) eq = eq && d[r.dims[k] * plane + pa] == d[r.dims[k] * plane + pb];
    return eq;
}

__device__ inline uint32_t div_tuple_slot(const long long* d, size_t plane, const DivRule& r, uint32_t p, uint32_t bits) {
    unsigned long long h = 0x243F6A8885A308D3ull;
    for (uint32_t k = 0; k < r.n_dims; ++k) {
        h = (h ^ (unsigned long long)d[r.dims[k] * plane + p]) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    return (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

__device__ inline uint32_t div_tab_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the first set bit of the waves' masks as a position of the chunk, kDivNone if there is none
__device__ inline uint32_t div_first(const unsigned long long* wm) {
    for (uint32_t w = 0; w < kDivWaves; ++w) {
        const unsigned long long m = wm[w];
        if (m) return w * kWave + (uint32_t)__builtin_ctzll(m);
    }
    return kDivNone;
}

// Request q = blockIdx.x.
__global__ __launch_bounds__(kDivThreads) void diversity_rules_kernel(DivArgs a) {
    __shared__ uint16_t cpos[kDivMaxN];          // kept entry j -> its position; the set-aside entries from the end, reversed
    __shared__ uint16_t res[kDivMaxN];           // the result, as kept-entry numbers
    __shared__ uint8_t exb[kDivMaxN];            // bit e: exclusion rule e's terms hold for kept entry j
    __shared__ uint32_t taken[kDivMaxN / 32];
    __shared__ unsigned long long welig[2][kDivWaves], wpass[kDivWaves], wbest[kDivWaves];
    __shared__ uint32_t wcnt[2][2][kDivWaves];   // [flag][set][wave]: the compaction's two flags; the output's walk uses flag 0's sets
    __shared__ uint32_t tail_key[kDivMaxRules], tail_run[kDivMaxRules];
    __shared__ uint32_t exm_s;                   // the exclusion rules that name the position being filled
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t cap = a.cap, n_rules = a.c.n_rules, n_excl = a.c.n_excl;
    const uint32_t n = a.count ? min(a.count[q], cap) : cap;
    uint32_t* order = a.order + (size_t)q * cap;
    const bool on = n_rules > 0 && (!a.enable || a.enable[q] != 0);
    for (uint32_t p = n + tid; p < cap; p += kDivThreads) order[p] = kDivNone;
    // compact: kept entries in order from the front, set-aside entries from the back
    uint32_t m = 0;
    if (on) {
        const uint8_t* source = a.c.exclude_mask && a.source ? a.source + (size_t)q * cap : nullptr;
        uint32_t n_sa = 0;
        for (uint32_t c0 = 0, it = 0; c0 < n; c0 += kDivChunk, ++it) {
            const uint32_t p = c0 + tid;
            bool keep = p < n, sa = false;
            if (keep && source) {
                const uint32_t s = source[p];
                sa = s < 32u && ((a.c.exclude_mask >> s) & 1u);
                keep = !sa;
            }
            uint32_t nk, ns;                     // (two flags, one barrier: chunk_rank's steps, the counts side by side)
            const uint32_t rk = wave_rank(keep, &nk), rs = wave_rank(sa, &ns);
            if (lane == 0) {
                wcnt[0][it & 1u][wave] = nk;
                wcnt[1][it & 1u][wave] = ns;
            }
            __syncthreads();
            uint32_t bk = 0, bs = 0, tk = 0, ts = 0;
            for (uint32_t w = 0; w < kDivWaves; ++w) {
                const uint32_t ck = wcnt[0][it & 1u][w], cs = wcnt[1][it & 1u][w];
                if (w < wave) {
                    bk += ck;
                    bs += cs;
                }
                tk += ck;
                ts += cs;
            }
            if (keep) cpos[m + bk + rk] = (uint16_t)p;
            if (sa) cpos[n - 1u - (n_sa + bs + rs)] = (uint16_t)p;
            m += tk;
            n_sa += ts;
        }
    }
    if (m == 0) {                                // no rules, a request switched off, nothing left: the identity
        for (uint32_t p = tid; p < n; p += kDivThreads) order[p] = p;
        return;
    }
    __syncthreads();
    const size_t plane = (size_t)a.nq * cap;
    const long long* dims = a.dims + (size_t)q * cap;
    uint32_t* keys = a.keys + (size_t)q * n_rules * cap;
    uint32_t* cnt = a.cnt + (size_t)q * n_rules * cap;
    uint32_t* tbl = a.tbl + ((size_t)q << a.slot_bits);
    const uint32_t slots = 1u << a.slot_bits, smask = slots - 1u;
    // keys: per rule, the smallest kept entry with an equal tuple
    for (uint32_t r = 0; r < n_rules; ++r) {
        const DivRule& ru = a.c.rules[r];
        for (uint32_t i = tid; i < slots; i += kDivThreads) __hip_atomic_store(&tbl[i], kDivNone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        for (uint32_t j = tid; j < m; j += kDivThreads) {
            const uint32_t p = cpos[j];
            for (uint32_t h = div_tuple_slot(dims, plane, ru, p, a.slot_bits);; h = (h + 1u) & smask) {
                uint32_t cur = div_tab_load(&tbl[h]);
                if (cur == kDivNone) cur = atomicCAS(&tbl[h], kDivNone, j);
                if (cur == kDivNone) break;                                  // claimed: the slot holds j
                if (cur < m && div_tuple_eq(dims, plane, ru, p, cpos[cur])) {
                    atomicMin(&tbl[h], j);
                    break;
                }
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < m; j += kDivThreads) {
            const uint32_t p = cpos[j];
            uint32_t key = j;
            for (uint32_t h = div_tuple_slot(dims, plane, ru, p, a.slot_bits);; h = (h + 1u) & smask) {
                const uint32_t cur = div_tab_load(&tbl[h]);
                if (cur >= m) break;                                         // (never: the tuple was inserted)
                if (div_tuple_eq(dims, plane, ru, p, cpos[cur])) {
                    key = cur;
                    break;
                }
            }
            keys[(size_t)r * cap + j] = key;
            cnt[(size_t)r * cap + j] = 0u;
        }
        __syncthreads();
    }
    // bits: the exclusion rules' terms
    for (uint32_t j = tid; j < m; j += kDivThreads) {
        const uint32_t p = cpos[j];
        uint32_t eb = 0;
        for (uint32_t e = 0; e < n_excl; ++e) {
            const DivExcl& ex = a.c.excl[e];
            bool all = true;
            for (uint32_t t = 0; t < ex.n_terms; ++t) all = all && div_term_holds(ex.terms[t].op, dims[ex.terms[t].column * plane + p], ex.terms[t].value);
            eb |= all ? 1u << e : 0u;
        }
        exb[j] = (uint8_t)eb;
    }
    for (uint32_t i = tid; i < kDivMaxN / 32; i += kDivThreads) taken[i] = 0u;
    if (tid < kDivMaxRules) {
        tail_key[tid] = kDivNone;
        tail_run[tid] = 0u;
    }
    // the exclusion rules that name a position: positions ascend, so does the position being filled — one cursor per rule
    uint32_t ex_cur = 0;
    auto excl_at = [&](uint32_t position) {      // wave 0 only
        bool hit = false;
        if (lane < n_excl) {
            const DivExcl& ex = a.c.excl[lane];
            while (ex_cur < ex.n_pos && ex.pos[ex_cur] < position) ++ex_cur;
            hit = ex_cur < ex.n_pos && ex.pos[ex_cur] == position;
        }
        const unsigned long long mm = __ballot(hit);
        if (lane == 0) exm_s = (uint32_t)mm;
    };
    if (wave == 0) excl_at(1u);
    __syncthreads();
    // greedy
    long long D = a.c.size;
    if (a.c.diversity_size > 0) D = min((long long)a.c.diversity_size, (long long)m);
    const bool has_weight = a.c.has_weight != 0;
    const uint32_t explore = a.c.explore > 0 ? (uint32_t)a.c.explore : 0u;
    uint32_t s = 0, lo = 0;                      // the result's length (= picks), the first untaken entry
    uint32_t it = 0;
    for (;;) {
        if (s > 0 && ((long long)s > D || s == m)) break;
        const uint32_t exm = exm_s;
        uint32_t f = kDivNone, bound = kDivNone, pick = kDivNone;
        unsigned long long best = 0ull;
        for (uint32_t c0 = lo & ~(kDivChunk - 1u); c0 < m; c0 += kDivChunk, ++it) {
            const uint32_t j = c0 + tid;
            const bool elig = j < m && !((taken[j >> 5] >> (j & 31u)) & 1u) && !(exb[j] & exm);
            const unsigned long long be = __ballot(elig);
            if (lane == 0) welig[it & 1u][wave] = be;
            __syncthreads();
            if (f == kDivNone) {
                const uint32_t at = div_first(welig[it & 1u]);
                if (at == kDivNone) continue;                                // every entry of the chunk is taken or skipped
                f = c0 + at;
                if (explore) bound = f + explore;
            }
            const bool inb = elig && j < bound;
            bool ok = inb;
            long long w = 0;
            if (inb) {
                for (uint32_t r = 0; r < n_rules; ++r) {
                    const DivRule& ru = a.c.rules[r];
                    const uint32_t k = keys[(size_t)r * cap + j];
                    bool fail = ru.interval > 0 && tail_key[r] == k && tail_run[r] >= (uint32_t)ru.interval;
                    if (ru.win_on) fail = fail || 1u + cnt[(size_t)r * cap + k] > (uint32_t)ru.frequency;
                    if (fail) ok = false;
                    else w += ru.weight;
                }
            }
            const unsigned long long bp = __ballot(ok);
            if (lane == 0) wpass[wave] = bp;
            if (has_weight) {
                // (w + 2^35) << 16 | (0xFFFF - j): the largest w, then the smallest j; 0 = not evaluated
                unsigned long long v = inb ? ((unsigned long long)(w + (1ll << 35)) << 16) | (0xFFFFull - j) : 0ull;
                for (int d = kWave / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, kWave));
                if (lane == 0) wbest[wave] = v;
            }
            __syncthreads();
            const uint32_t at = div_first(wpass);
            if (at != kDivNone) {
                pick = c0 + at;
                break;
            }
            if (has_weight)
                for (uint32_t wv = 0; wv < kDivWaves; ++wv) best = max(best, wbest[wv]);
            if (bound <= c0 + kDivChunk) break;                              // the explore bound ends the walk
        }
        if (pick == kDivNone) {
            if (f != kDivNone) pick = has_weight ? 0xFFFFu - (uint32_t)(best & 0xFFFFull) : f;
            else if (s == 0) pick = 0u;                                      // every entry is kept off position 1: entry 0
            else break;                                                      // every untaken entry was skipped
        }
        // the pick joins the result (every read of this step lies before a barrier)
        if (tid == 0) {
            taken[pick >> 5] |= 1u << (pick & 31u);
            res[s] = (uint16_t)pick;
        }
        if (tid < n_rules) {
            const DivRule& ru = a.c.rules[tid];
            uint32_t* kr = keys + (size_t)tid * cap;
            uint32_t* cr = cnt + (size_t)tid * cap;
            const uint32_t k = kr[pick];
            if (tail_key[tid] == k) {
                tail_run[tid] += 1u;
            } else {
                tail_key[tid] = k;
                tail_run[tid] = 1u;
            }
            if (ru.win_on) {                     // the window of the next step: [s + 2 - window, s + 1)
                cr[k] += 1u;
                const long long gone = (long long)s + 1 - ru.window;
                if (gone >= 0) cr[kr[res[gone]]] -= 1u;                      // (window >= 2: an earlier step's pick)
            }
        }
        if (wave == 0) excl_at(s + 2u);
        __syncthreads();
        ++s;
        while (lo < m && ((taken[lo >> 5] >> (lo & 31u)) & 1u)) ++lo;
    }
    // output: the result, the untaken entries in order, the set-aside entries in order
    for (uint32_t i = tid; i < s; i += kDivThreads) order[i] = cpos[res[i]];
    uint32_t base = s;
    for (uint32_t c0 = 0; c0 < m; c0 += kDivChunk, ++it) {
        const uint32_t j = c0 + tid;
        const bool left = j < m && !((taken[j >> 5] >> (j & 31u)) & 1u);
        uint32_t r, total;
        chunk_rank<kDivWaves>(left, wcnt[0][0], it, &r, &total);
        if (left) order[base + r] = cpos[j];
        base += total;
    }
    for (uint32_t t = tid; t < n - m; t += kDivThreads) order[m + t] = cpos[n - 1u - t];
}

// ---- the config ------------------------------------------------------------------------------------------------------------------

int div_check(const pg_div_config* cfg, uint32_t nq, uint32_t cap, bool have_source, const char* who, DivCfg* out) {
    PG_REQUIRE(cfg, "%s: NULL config", who);
    if (nq > (uint32_t)kMaxQueries) {
        set_error("%s: nq=%u unsupported (<= %d)", who, nq, kMaxQueries);
        return PG_ERR_UNSUPPORTED;
    }
    if (cap > kDivMaxN) {
        set_error("%s: cap=%u unsupported (<= PG_DIV_MAX_N = %u)", who, cap, kDivMaxN);
        return PG_ERR_UNSUPPORTED;
    }
    if (cfg->n_multi_value) {
        set_error("%s: MultiValueDimensionConf (list-valued dimensions) is not supported", who);
        return PG_ERR_UNSUPPORTED;
    }
    if (cfg->n_rules > kDivMaxRules || cfg->n_excl > kDivMaxExcl || cfg->n_cols > kDivMaxCols) {
        set_error("%s: n_rules=%u, n_excl=%u, n_cols=%u unsupported (<= %u, %u, %u)", who, cfg->n_rules, cfg->n_excl, cfg->n_cols, kDivMaxRules,
                  kDivMaxExcl, kDivMaxCols);
        return PG_ERR_UNSUPPORTED;
    }
    DivCfg c;
    memset(&c, 0, sizeof c);
    c.size = cfg->size;
    c.diversity_size = cfg->diversity_size;
    c.explore = cfg->explore_item_size;
    c.exclude_mask = cfg->exclude_source_mask;
    c.n_cols = cfg->n_cols;
    c.n_rules = cfg->n_rules;
    c.n_excl = cfg->n_excl;
    for (uint32_t r = 0; r < cfg->n_rules; ++r) {
        const pg_div_rule& in = cfg->rules[r];
        PG_REQUIRE(in.n_dims >= 1 && in.n_dims <= kDivMaxDims, "%s: rule %u has n_dims=%u (1..%u)", who, r, in.n_dims, kDivMaxDims);
        DivRule& ru = c.rules[r];
        ru.n_dims = in.n_dims;
        for (uint32_t k = 0; k < in.n_dims; ++k) {
            PG_REQUIRE(in.dims[k] < cfg->n_cols, "%s: rule %u names column index %u of n_cols=%u", who, r, in.dims[k], cfg->n_cols);
            ru.dims[k] = in.dims[k];
        }
        PG_REQUIRE(in.interval >= 0 && in.window >= 0 && in.frequency >= 0, "%s: rule %u has a negative interval, window or frequency (%d, %d, %d)",
                   who, r, in.interval, in.window, in.frequency);
        ru.interval = in.interval;
        ru.window = in.window;
        ru.frequency = in.frequency;
        ru.weight = in.weight;
        ru.win_on = in.window > 0 && in.frequency > 0 && in.window > in.frequency;
        if (in.weight > 0) c.has_weight = 1;
    }
    for (uint32_t e = 0; e < cfg->n_excl; ++e) {
        const pg_div_exclusion& in = cfg->excl[e];
        DivExcl& ex = c.excl[e];
        if (in.n_terms > kDivMaxTerms) {
            set_error("%s: exclusion rule %u has %u terms (<= %u)", who, e, in.n_terms, kDivMaxTerms);
            return PG_ERR_UNSUPPORTED;
        }
        PG_REQUIRE(in.n_terms >= 1, "%s: exclusion rule %u has no term", who, e);
        PG_REQUIRE(in.n_positions >= 1 && in.positions, "%s: exclusion rule %u has no position", who, e);
        ex.n_terms = in.n_terms;
        for (uint32_t t = 0; t < in.n_terms; ++t) {
            PG_REQUIRE(in.terms[t].column < cfg->n_cols, "%s: exclusion rule %u names column index %u of n_cols=%u", who, e, in.terms[t].column,
                       cfg->n_cols);
            PG_REQUIRE(in.terms[t].op >= PG_WHERE_GT && in.terms[t].op <= PG_WHERE_NE, "%s: exclusion rule %u has the unknown operator %d", who, e,
                       in.terms[t].op);
            ex.terms[t] = DivTerm{in.terms[t].column, in.terms[t].op, in.terms[t].value};
        }
        std::vector<uint32_t> pos;
        for (uint32_t i = 0; i < in.n_positions; ++i) {
            PG_REQUIRE(in.positions[i] != 0, "%s: exclusion rule %u names position 0 (positions are 1-based)", who, e);
            if (in.positions[i] <= kDivMaxN + 1u) pos.push_back(in.positions[i]);          // (others are never filled)
        }
        std::sort(pos.begin(), pos.end());
        pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
        if (pos.size() > kDivMaxPositions) {
            set_error("%s: exclusion rule %u names %zu positions (<= PG_DIV_MAX_POSITIONS = %u)", who, e, pos.size(), kDivMaxPositions);
            return PG_ERR_UNSUPPORTED;
        }
        ex.n_pos = (uint32_t)pos.size();
        for (size_t i = 0; i < pos.size(); ++i) ex.pos[i] = (uint16_t)pos[i];
    }
    PG_REQUIRE(!cfg->exclude_source_mask || have_source, "%s: exclude_source_mask needs source", who);
    *out = c;
    return PG_OK;
}

// ---- the host statement ----------------------------------------------------------------------------------------------------------

// one request; dims: column c of position i at dims[c * plane + i]
void div_host_one(const DivCfg& c, uint32_t n, uint32_t cap, const int64_t* dims, size_t plane, const uint8_t* source, bool on, uint32_t* order) {
    for (uint32_t p = n; p < cap; ++p) order[p] = kDivNone;
    std::vector<uint32_t> kept, aside;
    if (on && c.n_rules > 0)
        for (uint32_t p = 0; p < n; ++p) {
            const bool sa = c.exclude_mask && source && source[p] < 32 && ((c.exclude_mask >> source[p]) & 1u);
            (sa ? aside : kept).push_back(p);
        }
    const uint32_t m = (uint32_t)kept.size();
    if (m == 0) {
        for (uint32_t p = 0; p < n; ++p) order[p] = p;
        return;
    }
    // keys: the first kept entry with an equal tuple
    std::vector<std::vector<uint32_t>> keys(c.n_rules, std::vector<uint32_t>(m)), cnt(c.n_rules, std::vector<uint32_t>(m, 0u));
    std::vector<uint32_t> idx(m);
    for (uint32_t r = 0; r < c.n_rules; ++r) {
        const DivRule& ru = c.rules[r];
        auto less = [&](uint32_t x, uint32_t y) {
            for (uint32_t k = 0; k < ru.n_dims; ++k) {
                const int64_t vx = dims[ru.dims[k] * plane + kept[x]], vy = dims[ru.dims[k] * plane + kept[y]];
                if (vx != vy) return vx < vy;
            }
            return x < y;
        };
        auto same = [&](uint32_t x, uint32_t y) {
            for (uint32_t k = 0; k < ru.n_dims; ++k)
                if (dims[ru.dims[k] * plane + kept[x]] != dims[ru.dims[k] * plane + kept[y]]) return false;
            return true;
        };
        std::iota(idx.begin(), idx.end(), 0u);
        std::sort(idx.begin(), idx.end(), less);
        for (uint32_t i = 0, head = 0; i < m; ++i) {
            if (i > 0 && !same(idx[i], idx[head])) head = i;
            keys[r][idx[i]] = idx[head];
        }
    }
    std::vector<uint8_t> exb(m, 0);
    for (uint32_t j = 0; j < m; ++j)
        for (uint32_t e = 0; e < c.n_excl; ++e) {
            bool all = true;
            for (uint32_t t = 0; t < c.excl[e].n_terms; ++t)
                all = all && div_term_holds(c.excl[e].terms[t].op, dims[c.excl[e].terms[t].column * plane + kept[j]], c.excl[e].terms[t].value);
            if (all) exb[j] |= (uint8_t)(1u << e);
        }
    auto excl_at = [&](uint32_t position) {
        uint32_t mask = 0;
        for (uint32_t e = 0; e < c.n_excl; ++e)
            if (std::binary_search(c.excl[e].pos, c.excl[e].pos + c.excl[e].n_pos, (uint16_t)position) && position <= kDivMaxN + 1u) mask |= 1u << e;
        return mask;
    };
    std::vector<uint8_t> taken(m, 0);
    std::vector<uint32_t> res;
    res.reserve(m);
    uint32_t tail_key[kDivMaxRules], tail_run[kDivMaxRules];
    for (uint32_t r = 0; r < kDivMaxRules; ++r) {
        tail_key[r] = kDivNone;
        tail_run[r] = 0;
    }
    long long D = c.size;
    if (c.diversity_size > 0) D = std::min<long long>(c.diversity_size, m);
    uint32_t lo = 0;
    for (;;) {
        const uint32_t s = (uint32_t)res.size();
        if (s > 0 && ((long long)s > D || s == m)) break;
        const uint32_t exm = excl_at(s + 1u);
        uint32_t f = kDivNone, pick = kDivNone, best = kDivNone;
        long long best_w = 0;
        for (uint32_t j = lo; j < m; ++j) {
            if (taken[j] || (exb[j] & exm)) continue;
            if (f == kDivNone) f = j;
            if (c.explore > 0 && j - f >= (uint32_t)c.explore) break;
            bool ok = true;
            long long w = 0;
            for (uint32_t r = 0; r < c.n_rules; ++r) {
                const DivRule& ru = c.rules[r];
                const uint32_t k = keys[r][j];
                bool fail = ru.interval > 0 && tail_key[r] == k && tail_run[r] >= (uint32_t)ru.interval;
                if (ru.win_on) fail = fail || 1u + cnt[r][k] > (uint32_t)ru.frequency;
                if (fail) ok = false;
                else w += ru.weight;
                if (fail && !c.has_weight) break;
            }
            if (ok) {
                pick = j;
                break;
            }
            if (!c.has_weight) w = 0;
            if (best == kDivNone || w > best_w) {
                best = j;
                best_w = w;
            }
        }
        if (pick == kDivNone) {
            if (f != kDivNone) pick = best;
            else if (s == 0) pick = 0;
            else break;
        }
        taken[pick] = 1;
        res.push_back(pick);
        for (uint32_t r = 0; r < c.n_rules; ++r) {
            const DivRule& ru = c.rules[r];
            const uint32_t k = keys[r][pick];
            if (tail_key[r] == k) {
                ++tail_run[r];
            } else {
                tail_key[r] = k;
                tail_run[r] = 1;
            }
            if (ru.win_on) {
                ++cnt[r][k];
                const long long gone = (long long)s + 1 - ru.window;
                if (gone >= 0) --cnt[r][keys[r][res[(size_t)gone]]];
            }
        }
        while (lo < m && taken[lo]) ++lo;
    }
    uint32_t at = 0;
    for (uint32_t j : res) order[at++] = kept[j];
    for (uint32_t j = 0; j < m; ++j)
        if (!taken[j]) order[at++] = kept[j];
    for (uint32_t p : aside) order[at++] = p;
}

// caller holds ctx->mu; no synchronisation
int div_launch_locked(pg_ctx* ctx, const DivCfg& c, uint32_t nq, uint32_t cap, const uint32_t* d_count, const int64_t* d_dims,
                      const uint8_t* d_source, const uint8_t* d_enable, uint32_t* d_order) {
    if (nq == 0 || cap == 0) return PG_OK;
    uint32_t bits = 0;
    while ((1u << bits) < std::max(2u * cap, kDivMinSlots)) ++bits;
    const uint32_t nr = std::max(c.n_rules, 1u);
    DivArgs a;
    memset(&a, 0, sizeof a);
    int rc;
    if ((rc = scratch_carve(ctx, kSlotDiversity, [&](Carve& s) {
            a.keys = s.take<uint32_t>((size_t)nq * nr * cap);
            a.cnt = s.take<uint32_t>((size_t)nq * nr * cap);
            a.tbl = s.take<uint32_t>((size_t)nq << bits);
        }))) return rc;
    a.c = c;
    a.dims = reinterpret_cast<const long long*>(d_dims);
    a.source = d_source;
    a.count = d_count;
    a.enable = d_enable;
    a.order = d_order;
    a.nq = nq;
    a.cap = cap;
    a.slot_bits = bits;
    diversity_rules_kernel<<<nq, kDivThreads, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

struct DivCols {
    const void* base[kDivMaxCols];
    long long def[kDivMaxCols];
    uint32_t is64;                               // bit c: column c is int64
    uint64_t rows;
    uint32_t n_cols;
};

// planes[(c * nq + q) * cap + i] = column c at rows[q][i], the column default for a row outside the store
__global__ void diversity_gather_kernel(DivCols cols, const uint64_t* __restrict__ rows, size_t n, long long* __restrict__ planes) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = rows[i];
    for (uint32_t c = 0; c < cols.n_cols; ++c) {
        long long v = cols.def[c];
        if (row < cols.rows) v = (cols.is64 >> c) & 1u ? ((const long long*)cols.base[c])[row] : (long long)((const int32_t*)cols.base[c])[row];
        planes[(size_t)c * n + i] = v;
    }
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_diversity_rules_host(const pg_div_config* cfg, uint32_t nq, uint32_t cap, const uint32_t* count, const int64_t* dims,
                            const uint8_t* source, const uint8_t* enable, uint32_t* order) {
    pg::DivCfg c;
    int rc;
    if ((rc = pg::div_check(cfg, nq, cap, source != nullptr, "pg_diversity_rules_host", &c))) return rc;
    if (nq == 0 || cap == 0) return PG_OK;
    PG_REQUIRE(order && (dims || c.n_cols == 0), "pg_diversity_rules_host: NULL argument");
    const size_t plane = (size_t)nq * cap;
    auto one = [&](uint32_t q) {
        const uint32_t n = count ? std::min(count[q], cap) : cap;
        pg::div_host_one(c, n, cap, dims + (size_t)q * cap, plane, source ? source + (size_t)q * cap : nullptr, !enable || enable[q] != 0,
                         order + (size_t)q * cap);
    };
    const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    const uint32_t nt = std::min({nq, hw, 16u});
    if (nt <= 1) {
        for (uint32_t q = 0; q < nq; ++q) one(q);
        return PG_OK;
    }
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            for (uint32_t q = t; q < nq; q += nt) one(q);
        });
    for (auto& x : th) x.join();
    return PG_OK;
}

int pg_diversity_rules_dev(pg_ctx* ctx, const pg_div_config* cfg, uint32_t nq, uint32_t cap, const uint32_t* d_count,
                           const int64_t* d_dims, const uint8_t* d_source, const uint8_t* d_enable, uint32_t* d_order) {
    PG_REQUIRE(ctx, "pg_diversity_rules_dev: NULL context");
    pg::DivCfg c;
    int rc;
    if ((rc = pg::div_check(cfg, nq, cap, d_source != nullptr, "pg_diversity_rules_dev", &c))) return rc;
    PG_REQUIRE(nq == 0 || cap == 0 || (d_order && (d_dims || c.n_cols == 0)), "pg_diversity_rules_dev: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::div_launch_locked(ctx, c, nq, cap, d_count, d_dims, d_source, d_enable, d_order);
}

int pg_diversity_rules_features_dev(pg_ctx* ctx, const pg_div_config* cfg, const pg_features* fs, const char* const* col_names,
                                    uint32_t nq, uint32_t cap, const uint64_t* d_rows, const uint32_t* d_count,
                                    const uint8_t* d_source, const uint8_t* d_enable, uint32_t* d_order) {
    PG_REQUIRE(ctx && fs, "pg_diversity_rules_features_dev: NULL argument");
    pg::DivCfg c;
    int rc;
    if ((rc = pg::div_check(cfg, nq, cap, d_source != nullptr, "pg_diversity_rules_features_dev", &c))) return rc;
    PG_REQUIRE(col_names || c.n_cols == 0, "pg_diversity_rules_features_dev: NULL column names");
    pg::DivCols cols;
    memset(&cols, 0, sizeof cols);
    cols.rows = fs->rows;
    cols.n_cols = c.n_cols;
    for (uint32_t k = 0; k < c.n_cols; ++k) {
        PG_REQUIRE(col_names[k], "pg_diversity_rules_features_dev: column name %u is NULL", k);
        const int ci = pg_features_column_index(fs, col_names[k]);
        PG_REQUIRE(ci >= 0, "pg_diversity_rules_features_dev: the feature store has no column \"%s\"", col_names[k]);
        const pg_features::Column& col = fs->cols[(size_t)ci];
        PG_REQUIRE(col.dtype == PG_F_I32 || col.dtype == PG_F_I64, "pg_diversity_rules_features_dev: column \"%s\" must be int32 / int64", col_names[k]);
        PG_REQUIRE(col.d, "pg_diversity_rules_features_dev: column \"%s\" has no values", col_names[k]);
        cols.base[k] = col.d;
        cols.def[k] = (long long)col.def;
        if (col.dtype == PG_F_I64) cols.is64 |= 1u << k;
    }
    PG_REQUIRE(nq == 0 || cap == 0 || (d_order && d_rows), "pg_diversity_rules_features_dev: NULL argument");
    if (nq == 0 || cap == 0) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)nq * cap;
    void* planes;
    if ((rc = pg::scratch_reserve(ctx, pg::kSlotDiversityPlanes, std::max<size_t>((size_t)c.n_cols * n * 8, 256), &planes))) return rc;
    if (c.n_cols) {
        pg::diversity_gather_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(cols, d_rows, n, (long long*)planes);
        PG_HIP(hipGetLastError());
    }
    return pg::div_launch_locked(ctx, c, nq, cap, d_count, (const int64_t*)planes, d_source, d_enable, d_order);
}

int pg_diversity_rules(pg_ctx* ctx, const pg_div_config* cfg, uint32_t n, const int64_t* dims, const uint8_t* source, uint32_t* order) {
    PG_REQUIRE(ctx, "pg_diversity_rules: NULL context");
    pg::DivCfg c;
    int rc;
    if ((rc = pg::div_check(cfg, 1, n, source != nullptr, "pg_diversity_rules", &c))) return rc;
    if (n == 0) return PG_OK;
    PG_REQUIRE(order && (dims || c.n_cols == 0), "pg_diversity_rules: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kDims, kSource, kOrder };
    Staged st[] = {{dims, (size_t)c.n_cols * n * 8, Staged::kIn}, {source, n, Staged::in_if(source)}, {order, (size_t)n * 4, Staged::kOut}};
    return pg::staged_run(ctx, pg::kSlotStaging, st, sizeof st / sizeof *st, false, [&] {
        return pg::div_launch_locked(ctx, c, 1, n, nullptr, st[kDims].at<int64_t>(), source ? st[kSource].at<uint8_t>() : nullptr, nullptr,
                                     st[kOrder].at<uint32_t>());
    });
}

}  // extern "C"
