// mixsort.hip — MultiRecallMixSort on the device: the reference's page-shaping sort behind ItemRankScore
// (sort/multi_recall_mix_sort.go:62-178, sort/mix_sort_strategy.go).  Every MixSortConfig is a strategy that claims entries by
// recall name or by a module.FilterParam, then puts them at configured positions of the page (fix_position, BuildItems :137-155)
// or at a random place of each stride (random_position, :178-216); the default strategy and remainItemIterator (:180-216) fill
// the rest.  include/pairec_gpu.h states the answer step by step (pg_mix_sort_dev); the numbers of the steps below are its.
//
// The reference walks item by item with the strategies inside and stops once every list is full (:82-128).  A strategy takes
// every member it meets until it is full, and an item goes to the first strategy that is not full, so strategy s holds the first
// number_s members no earlier strategy took: the lists can be built strategy by strategy against a bitmap of taken entries, which
// is classcut.hip's cut.  After UniqueFilter ids are unique, so remainItemIterator's id map is a flag per list position.
//
//   mix_match_kernel   one lane per list entry: its element (through d_order), its row, every referenced column's raw value (all
//                      loads issued before the first use, cond_eval.hpp), then per strategy the source-mask test ORed with the
//                      strategy's FilterParam rule → one byte, bit s = member of strategy s.  256 lanes, grid (cap / 256, nq).
//   mix_sort_kernel    one workgroup of 1 024 lanes per request.  Strategies in turn walk the list 1 024 entries at a time:
//                      block_rank.hpp's chunk_rank (one barrier per chunk; all walks share one counter) and the running count give a
//                      member its rank; a 2 KB LDS bitmap records taken entries; the walk ends in the chunk where the rank reaches
//                      number_s.  The taken lists (and, for a position column, the entries' column values) go to global scratch.
//                      Wave 0 then places FIX and RANDOM entries into the page in LDS: it reads lists and positions 64 at a time
//                      and walks them in order with the page's occupancy in registers (lane l holds slots [64 l, 64 l + 64)), so
//                      "a later write replaces" and "the first empty slot from `end` on" are statements about one wave's program
//                      order.  All lanes then derive the "in result" bitmap from the page, compact the empty slots, and fill
//                      them by ballot rank: first from the entries nobody took (D), then from the entries not in the page.  The
//                      tail is one more ranked walk.  Nothing depends on which lane came first.
#include "pipeline.hpp"
#include "cond_eval.hpp"
#include "block_rank.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <memory>
#include <thread>

namespace pg {
namespace {

constexpr uint32_t kMixMaxStrategies = 8, kMixMaxPositions = 256, kMixMaxSize = 4096;
constexpr uint32_t kMixChunk = 1024, kMixWaves = kMixChunk / kWave, kMixMatchThreads = 256;
constexpr uint32_t kMixEmpty = 0xFFFFFFFFu, kMixNoRule = 0xFFu;
static_assert(kMixMaxStrategies == PG_MIX_MAX_STRATEGIES && kMixMaxPositions == PG_MIX_MAX_POSITIONS && kMixMaxSize == PG_MIX_MAX_SIZE &&
                  kMixChunk == PG_TRIM_CHUNK,
              "include/pairec_gpu.h repeats these");
static_assert(kMixMaxStrategies <= 8, "a member mask is one byte");
static_assert(kMixMaxSize == kWave * 64, "wave 0 holds the page's occupancy as one 64-bit word per lane");
static_assert(kCandMaxCap / 32 == 512, "the bitmaps of list positions are 2 KB");

// draw(q, s, j) of step 5: the splitmix64 finaliser of seed + golden * (1 + s * 65536 + j)
__host__ __device__ __forceinline__ unsigned long long mix_draw(unsigned long long seed, uint32_t s, uint32_t j) {
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * (1ull + (unsigned long long)s * 65536ull + j);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// a position column's value as steps 4 keeps it: p in [1, S], or -1 for "places nothing" (p <= 0, p > S, a missing row)
__host__ __device__ __forceinline__ int32_t mix_pos_value(long long v, uint32_t S) { return v > 0 && v <= (long long)S ? (int32_t)v : -1; }

struct MixStrat {                          // one strategy at the call's S
    uint32_t type, number, keep, off;      // keep: the entries of its list that are stored, at [off, off + keep) of the request's lists
    uint32_t pos_off, n_pos;               // FIX: its configured positions in the set's table
    const void* pos_col;                   // FIX without positions: its position column in the store (or nullptr)
    uint32_t pos_i64, src_mask, rule, pad; // rule: its FilterParam in the cond set (kMixNoRule: no conditions)
};
struct MixArgs {
    MixStrat st[kMixMaxStrategies];
    uint32_t n_st, S, remain, cap, keep_total, pad;
    unsigned long long store_rows;
    const uint64_t* rows;                  // [nq][cap] by element
    const uint8_t* source;                 // [nq][cap] by element, or nullptr
    const uint32_t* order;                 // [nq][cap] list entry → element, or nullptr
    const uint32_t* count;                 // [nq] or nullptr
    const unsigned long long* seed;        // [nq] or nullptr
    const unsigned long long* user_vals;   // [nq][kCondMaxSlots] or nullptr
    const uint32_t* user_present;          // [nq] or nullptr
    const int32_t* pos_table;              // the set's configured positions
    uint8_t* mask;                         // [nq][cap] by list entry
    uint32_t* taken;                       // [nq][keep_total] list entries
    int32_t* taken_pos;                    // [nq][keep_total] mix_pos_value of the entry's position column
    uint32_t* out_order;                   // [nq][cap]
    uint32_t* out_count;                   // [nq]
};

// Request q = blockIdx.y, list entries blockIdx.x * 256 ...
__global__ __launch_bounds__(kMixMatchThreads) void mix_match_kernel(CondProgram p, MixArgs a) {
    const uint32_t q = blockIdx.y, j = blockIdx.x * kMixMatchThreads + threadIdx.x;
    if (j >= a.cap) return;
    const size_t q0 = (size_t)q * a.cap;
    const uint32_t n = a.count ? min(a.count[q], a.cap) : a.cap;
    uint32_t bits = 0;
    const uint32_t elem = j < n ? (a.order ? a.order[q0 + j] : j) : a.cap;
    if (elem < a.cap) {                                             // (an order value outside the arrays is a member of nothing)
        CondUser u;
        u.vals = a.user_vals ? a.user_vals + (size_t)q * kCondMaxSlots : nullptr;
        u.present = a.user_present ? a.user_present[q] : 0u;
        const uint32_t src = a.source ? a.source[q0 + elem] : 0xFFu;
        CondItem item;
        cond_load(p, a.rows[q0 + elem], &item);
        for (uint32_t s = 0; s < a.n_st; ++s) {
            bool mem = src < 32u && ((a.st[s].src_mask >> src) & 1u) != 0;
            if (!mem && a.st[s].rule != kMixNoRule) mem = cond_rule(p, a.st[s].rule, item, u);
            bits |= mem ? 1u << s : 0u;
        }
    }
    a.mask[q0 + j] = (uint8_t)bits;                                  // every byte of [nq][cap] is written
}

__device__ __forceinline__ bool mix_bit(const uint32_t* bm, uint32_t j) { return ((bm[j >> 5] >> (j & 31u)) & 1u) != 0; }
__device__ __forceinline__ void mix_set(uint32_t* bm, uint32_t j) { atomicOr(&bm[j >> 5], 1u << (j & 31u)); }

// wave 0: the first empty slot from `end` on, cyclically; free = the lane's empty slots; at least one slot of the page is empty
__device__ __forceinline__ uint32_t mix_first_empty(unsigned long long free, uint32_t end, uint32_t lane) {
    const uint32_t el = end >> 6;
    const unsigned long long from = ~0ull << (end & 63u);
    unsigned long long c = lane > el ? free : lane == el ? (free & from) : 0ull;
    unsigned long long b = __ballot(c != 0ull);
    if (b == 0ull) {                                                 // (wave-uniform) wrap round to the slots in front of `end`
        c = lane < el ? free : lane == el ? (free & ~from) : 0ull;
        b = __ballot(c != 0ull);
    }
    const uint32_t l = (uint32_t)__builtin_ctzll(b);
    const uint32_t bit = c ? (uint32_t)__builtin_ctzll(c) : 0u;
    return l * 64u + (uint32_t)__shfl((int)bit, (int)l);
}

// Request q = blockIdx.x.
__global__ __launch_bounds__(kMixChunk) void mix_sort_kernel(MixArgs a) {
    __shared__ uint32_t s_res[kMixMaxSize];                          // the page: list entries, kMixEmpty for an empty slot
    __shared__ uint32_t s_empty[kMixMaxSize];                        // the empty slots after FIX and RANDOM, ascending
    __shared__ uint32_t s_taken[kCandMaxCap / 32], s_inres[kCandMaxCap / 32];
    __shared__ uint32_t s_wcnt[2 * kMixWaves];
    __shared__ uint32_t s_cnt[kMixMaxStrategies];                    // |taken_s|
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const size_t q0 = (size_t)q * a.cap;
    const uint32_t n = a.count ? min(a.count[q], a.cap) : a.cap, S = a.S;
    const uint32_t* ord = a.order ? a.order + q0 : nullptr;
    uint32_t* out = a.out_order + q0;
    if (n < S) {                                                     // 1. a short list stays as it is
        for (uint32_t j = tid; j < a.cap; j += kMixChunk) out[j] = j < n ? (ord ? ord[j] : j) : kMixEmpty;
        if (tid == 0) a.out_count[q] = n;
        return;
    }
    for (uint32_t w = tid; w < kCandMaxCap / 32; w += kMixChunk) { s_taken[w] = 0; s_inres[w] = 0; }
    for (uint32_t slot = tid; slot < S; slot += kMixChunk) s_res[slot] = kMixEmpty;
    __syncthreads();
    const uint8_t* mask = a.mask + q0;
    uint32_t* tk = a.taken + (size_t)q * a.keep_total;
    int32_t* tp = a.taken_pos + (size_t)q * a.keep_total;
    uint32_t it = 0;

    // 3. taken_s: the first number_s members no earlier strategy took
    for (uint32_t s = 0; s < a.n_st; ++s) {
        const MixStrat& st = a.st[s];
        uint32_t run = 0;
        for (uint32_t c0 = 0; c0 < n && run < st.number; c0 += kMixChunk) {
            const uint32_t j = c0 + tid;
            const bool mem = j < n && ((mask[j] >> s) & 1u) != 0 && !mix_bit(s_taken, j);
            uint32_t r, total;
            chunk_rank<kMixWaves>(mem, s_wcnt, it++, &r, &total);
            r += run;
            if (mem && r < st.number) {
                mix_set(s_taken, j);
                if (r < st.keep) {
                    tk[st.off + r] = j;
                    if (st.pos_col) {
                        const uint32_t elem = ord ? ord[j] : j;
                        long long v = -1;
                        if (elem < a.cap) {
                            const unsigned long long row = a.rows[q0 + elem];
                            if (row < a.store_rows) v = st.pos_i64 ? ((const long long*)st.pos_col)[row] : (long long)((const int32_t*)st.pos_col)[row];
                        }
                        tp[st.off + r] = mix_pos_value(v, S);
                    }
                }
            }
            run += total;
        }
        if (tid == 0) s_cnt[s] = min(run, st.number);
        __syncthreads();                                             // the next strategy reads this one's bits; wave 0 reads the lists
    }

    // 4. and 5.: wave 0 places, in program order
    if (wave == 0) {
        const uint32_t lo = lane * 64u;
        const uint32_t nb = S > lo ? min(64u, S - lo) : 0u;
        const unsigned long long valid = nb == 64u ? ~0ull : ((1ull << nb) - 1ull);
        unsigned long long occ = 0;                                  // the lane's occupied slots
        for (uint32_t s = 0; s < a.n_st; ++s) {
            const MixStrat& st = a.st[s];
            if (st.type != PG_MIX_FIX) continue;
            const uint32_t cnt = min(s_cnt[s], st.keep);
            const uint32_t n_p = st.n_pos ? st.n_pos : st.pos_col ? cnt : 0u;
            uint32_t idx = 0, tbase = 0;
            uint32_t tb = lane < cnt ? tk[st.off + lane] : 0u;
            for (uint32_t b = 0; b < n_p && idx < cnt; b += kWave) {
                int32_t p = -1;
                if (b + lane < n_p) p = st.n_pos ? a.pos_table[st.pos_off + b + lane] : tp[st.off + b + lane];
                const uint32_t m = min((uint32_t)kWave, n_p - b);
                for (uint32_t t = 0; t < m && idx < cnt; ++t) {
                    const int32_t pt = __shfl(p, (int)t);
                    if (pt < 1 || (uint32_t)pt > S) continue;
                    if (idx >= tbase + kWave) {
                        tbase += kWave;
                        tb = tbase + lane < cnt ? tk[st.off + tbase + lane] : 0u;
                    }
                    const uint32_t e = (uint32_t)__shfl((int)tb, (int)(idx - tbase));
                    const uint32_t slot = (uint32_t)pt - 1u;
                    if (lane == 0) s_res[slot] = e;                  // (one lane, program order: a later write replaces)
                    if (lane == (slot >> 6)) occ |= 1ull << (slot & 63u);
                    ++idx;
                }
            }
        }
        uint32_t n_empty = (uint32_t)__popcll(~occ & valid);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_empty += (uint32_t)__shfl_xor((int)n_empty, o);
        const unsigned long long seed = a.seed ? a.seed[q] : 0ull;
        for (uint32_t s = 0; s < a.n_st; ++s) {
            const MixStrat& st = a.st[s];
            if (st.type != PG_MIX_RANDOM) continue;
            const uint32_t cnt = min(s_cnt[s], st.keep);
            if (cnt == 0) continue;
            const uint32_t step = S / st.number;                     // (number_s in [1, S]: the host refused the rest)
            uint32_t start = 0;
            for (uint32_t b = 0; b < cnt && n_empty; b += kWave) {
                const uint32_t tb = b + lane < cnt ? tk[st.off + b + lane] : 0u;
                const uint32_t m = min((uint32_t)kWave, cnt - b);
                for (uint32_t t = 0; t < m && n_empty; ++t) {
                    const uint32_t end = min(start + (uint32_t)(mix_draw(seed, s, b + t) % step), S - 1u);
                    const uint32_t slot = mix_first_empty(~occ & valid, end, lane);
                    const uint32_t e = (uint32_t)__shfl((int)tb, (int)t);
                    if (lane == 0) s_res[slot] = e;
                    if (lane == (slot >> 6)) occ |= 1ull << (slot & 63u);
                    --n_empty;
                    start += step;
                }
            }
        }
    }
    __syncthreads();

    // the "in result" bitmap from the page as it stands (a displaced entry is not in it), and the empty slots in order
    uint32_t n_e = 0;
    for (uint32_t c0 = 0; c0 < S; c0 += kMixChunk) {
        const uint32_t slot = c0 + tid;
        const uint32_t e = slot < S ? s_res[slot] : 0u;
        const bool empty = slot < S && e == kMixEmpty;
        if (slot < S && !empty) mix_set(s_inres, e);
        uint32_t r, total;
        chunk_rank<kMixWaves>(empty, s_wcnt, it++, &r, &total);
        if (empty) s_empty[n_e + r] = slot;
        n_e += total;
    }
    __syncthreads();

    // 6. D, the entries nobody took, into the empty slots
    uint32_t d_run = 0;
    for (uint32_t c0 = 0; c0 < n && d_run < n_e; c0 += kMixChunk) {
        const uint32_t j = c0 + tid;
        const bool free = j < n && !mix_bit(s_taken, j);
        uint32_t r, total;
        chunk_rank<kMixWaves>(free, s_wcnt, it++, &r, &total);
        r += d_run;
        if (free && r < n_e) {
            s_res[s_empty[r]] = j;
            mix_set(s_inres, j);
        }
        d_run += total;
    }
    d_run = min(d_run, n_e);
    __syncthreads();

    // 7. slots still empty: the entries not in the page, in list order (taken entries that were displaced or never placed)
    const uint32_t need = n_e - d_run;
    uint32_t r_run = 0;
    for (uint32_t c0 = 0; c0 < n && r_run < need; c0 += kMixChunk) {
        const uint32_t j = c0 + tid;
        const bool left = j < n && !mix_bit(s_inres, j);
        uint32_t r, total;
        chunk_rank<kMixWaves>(left, s_wcnt, it++, &r, &total);
        r += r_run;
        if (left && r < need) {
            s_res[s_empty[d_run + r]] = j;
            mix_set(s_inres, j);
        }
        r_run += total;
    }
    __syncthreads();

    // 8. the page, the tail, the padding
    for (uint32_t slot = tid; slot < S; slot += kMixChunk) {
        const uint32_t j = s_res[slot];
        out[slot] = j < n ? (ord ? ord[j] : j) : kMixEmpty;          // (j < n always: n >= S fills every slot)
    }
    uint32_t cnt_out = S;
    if (a.remain) {
        for (uint32_t c0 = 0; c0 < n; c0 += kMixChunk) {
            const uint32_t j = c0 + tid;
            const bool left = j < n && !mix_bit(s_inres, j);
            uint32_t r, total;
            chunk_rank<kMixWaves>(left, s_wcnt, it++, &r, &total);
            if (left && cnt_out + r < a.cap) out[cnt_out + r] = ord ? ord[j] : j;      // (cnt_out + r < n <= cap)
            cnt_out += total;
        }
        cnt_out = min(cnt_out, a.cap);
    }
    for (uint32_t j = cnt_out + tid; j < a.cap; j += kMixChunk) out[j] = kMixEmpty;
    if (tid == 0) a.out_count[q] = cnt_out;
}

}  // namespace
}  // namespace pg

// ---- the compiled object ------------------------------------------------------------------------------------------------------
struct pg_mix {
    struct Strategy {
        int type = 0;
        std::vector<int32_t> positions;               // FIX: as configured (every one >= 1)
        uint32_t pos_off = 0;                         // ... in pos_table
        int pos_decl = -1;                            // FIX without positions: the declared column behind position_field
        uint32_t number = 0;                          // Number (>= 0)
        double rate = 0.0;                            // NumberRate (>= 0)
        uint32_t src_mask = 0;
        uint32_t rule = pg::kMixNoRule;               // its FilterParam in `cond`
    };
    std::vector<Strategy> st;
    uint32_t size = 0, remain = 0;
    std::vector<std::string> col_names;               // as declared
    std::vector<int> col_dtypes;
    pg_cond* cond = nullptr;                          // the strategies' Conditions, one rule per strategy that has any (or nullptr)
    std::vector<int32_t> pos_table;
    pg::SetTable table;                               // the configured positions
    ~pg_mix() { pg_cond_free(cond); }
};

namespace pg {
namespace {

int mix_refuse(int code, const char* who, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int mix_refuse(int code, const char* who, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error("%s: %s", who, buf);
    return code;
}

// S and every number_s of a call (mix_sort_strategy.go:121-176)
int mix_numbers(const pg_mix* m, uint32_t ctx_size, const char* who, uint32_t* S_out, uint32_t* number) {
    const uint32_t S = std::max(ctx_size, m->size);
    if (S < 1) return mix_refuse(PG_ERR_INVALID, who, "the page size max(ctx_size, size) is 0");
    if (S > kMixMaxSize) return mix_refuse(PG_ERR_UNSUPPORTED, who, "page size %u (max(ctx_size, size)) unsupported (at most %u)", S, kMixMaxSize);
    for (size_t s = 0; s < m->st.size(); ++s) {
        const pg_mix::Strategy& st = m->st[s];
        if (st.type == PG_MIX_FIX) {
            number[s] = !st.positions.empty() ? (uint32_t)st.positions.size() : st.number;
        } else {
            if (st.rate > 0.0) {
                const double v = (double)S * st.rate;
                if (!(v <= (double)S))
                    return mix_refuse(PG_ERR_INVALID, who, "strategy %zu: random_position with number_rate %g asks for more than the page's %u slots "
                                      "(the reference's rand.Intn(0) panics)", s, st.rate, S);
                number[s] = (uint32_t)(int)v;
            } else {
                number[s] = st.number;
            }
            if (number[s] > S)
                return mix_refuse(PG_ERR_INVALID, who, "strategy %zu: random_position with number %u above the page's %u slots (the reference's "
                                  "rand.Intn(0) panics)", s, number[s], S);
        }
    }
    *S_out = S;
    return PG_OK;
}

int mix_check_call(const pg_mix* m, uint32_t nq, uint32_t cap, const void* source, const void* user_vals, const void* user_present, const char* who) {
    if (nq < 1 || nq > (uint32_t)kMaxQueries) return mix_refuse(nq < 1 ? PG_ERR_INVALID : PG_ERR_UNSUPPORTED, who, "nq=%u must be in [1,%d]", nq, kMaxQueries);
    if (cap < 1 || cap > kCandMaxCap) return mix_refuse(PG_ERR_UNSUPPORTED, who, "cap=%u unsupported (1..%u)", cap, kCandMaxCap);
    for (size_t s = 0; s < m->st.size(); ++s)
        if (m->st[s].src_mask && !source)
            return mix_refuse(PG_ERR_INVALID, who, "strategy %zu has a source mask (recall names) but the entries' source is NULL", s);
    if (m->cond && pg_cond_num_user_slots(m->cond) > 0 && !(user_vals && user_present))
        return mix_refuse(PG_ERR_INVALID, who, "the conditions read user property \"%s\": user_vals and user_present are needed",
                          pg_cond_user_slot_name(m->cond, 0));
    return PG_OK;
}

// the host statement for one request; member[j]: the strategy bits of list entry j, pos[s][j]: its position-column value
void mix_host_request(const pg_mix* m, uint32_t S, const uint32_t* number, uint32_t n, uint32_t cap, const uint8_t* member,
                      const std::vector<std::vector<int32_t>>& pos, const uint32_t* order, unsigned long long seed, uint32_t* out, uint32_t* out_count) {
    auto elem = [&](uint32_t j) { return order ? order[j] : j; };
    if (n < S) {
        for (uint32_t j = 0; j < cap; ++j) out[j] = j < n ? elem(j) : kMixEmpty;
        *out_count = n;
        return;
    }
    const size_t ns = m->st.size();
    std::vector<uint8_t> taken(n, 0), inres(n, 0);
    std::vector<std::vector<uint32_t>> lists(ns);
    for (size_t s = 0; s < ns; ++s)
        for (uint32_t j = 0; j < n && lists[s].size() < number[s]; ++j)
            if (((member[j] >> s) & 1u) && !taken[j]) {
                taken[j] = 1;
                lists[s].push_back(j);
            }
    std::vector<uint32_t> res(S, kMixEmpty);
    for (size_t s = 0; s < ns; ++s) {
        const pg_mix::Strategy& st = m->st[s];
        if (st.type != PG_MIX_FIX) continue;
        std::vector<int32_t> P;
        if (!st.positions.empty()) P = st.positions;
        else if (st.pos_decl >= 0)
            for (size_t j = 0; j < lists[s].size(); ++j)              // (j < min(number_s, |taken_s|): the list is no longer)
                if (pos[s][lists[s][j]] > 0) P.push_back(pos[s][lists[s][j]]);
        size_t idx = 0;
        for (int32_t p : P)
            if ((uint32_t)p <= S && idx < lists[s].size()) res[(size_t)p - 1] = lists[s][idx++];
    }
    uint32_t n_empty = 0;
    for (uint32_t e : res) n_empty += e == kMixEmpty;
    for (size_t s = 0; s < ns; ++s) {
        if (m->st[s].type != PG_MIX_RANDOM || lists[s].empty()) continue;
        const uint32_t step = S / number[s];
        uint32_t start = 0;
        for (size_t j = 0; j < lists[s].size() && n_empty; ++j) {
            uint32_t end = std::min(start + (uint32_t)(mix_draw(seed, (uint32_t)s, (uint32_t)j) % step), S - 1);
            while (res[end] != kMixEmpty) end = (end + 1) % S;
            res[end] = lists[s][j];
            --n_empty;
            start += step;
        }
    }
    for (uint32_t e : res)
        if (e != kMixEmpty) inres[e] = 1;
    uint32_t slot = 0;
    auto next_empty = [&] {
        while (slot < S && res[slot] != kMixEmpty) ++slot;
        return slot < S;
    };
    for (uint32_t j = 0; j < n; ++j)                                   // D (at most S of them are looked at: every one fills a slot)
        if (!taken[j]) {
            if (!next_empty()) break;
            res[slot] = j;
            inres[j] = 1;
        }
    for (uint32_t j = 0; j < n; ++j)                                   // the entries not in the page
        if (!inres[j]) {
            if (!next_empty()) break;
            res[slot] = j;
            inres[j] = 1;
        }
    uint32_t c = 0;
    for (; c < S; ++c) out[c] = res[c] < n ? elem(res[c]) : kMixEmpty;
    if (m->remain)
        for (uint32_t j = 0; j < n && c < cap; ++j)
            if (!inres[j]) out[c++] = elem(j);
    *out_count = c;
    for (; c < cap; ++c) out[c] = kMixEmpty;
}

// binds the set to a store and launches; caller holds ctx->mu.  d_* as pg_mix_sort_dev takes them.
int mix_sort_locked(pg_ctx* ctx, pg_mix* m, const pg_features* fs, uint32_t S, const uint32_t* number, uint32_t nq, uint32_t cap,
                    const uint64_t* d_rows, const uint8_t* d_source, const uint32_t* d_order, const uint32_t* d_count, const uint64_t* d_seed,
                    const uint64_t* d_user_vals, const uint32_t* d_user_present, uint32_t* d_out_order, uint32_t* d_out_count, const char* who) {
    int rc;
    MixArgs a{};
    CondProgram p;
    memset(&p, 0, sizeof p);
    if (m->cond && (rc = cond_bind_locked(ctx, m->cond, fs, who, &p))) return rc;
    uint32_t off = 0;
    for (size_t s = 0; s < m->st.size(); ++s) {
        const pg_mix::Strategy& st = m->st[s];
        MixStrat& o = a.st[s];
        o.type = (uint32_t)st.type;
        o.number = number[s];
        o.keep = std::min(number[s], cap);
        o.off = off;
        off += o.keep;
        o.pos_off = st.pos_off;
        o.n_pos = (uint32_t)st.positions.size();
        o.src_mask = st.src_mask;
        o.rule = st.rule;
        if (st.pos_decl >= 0) {
            const std::string& name = m->col_names[(size_t)st.pos_decl];
            const pg_features::Column* col = nullptr;
            for (const auto& x : fs->cols)
                if (x.name == name) { col = &x; break; }
            if (!col || !col->d) return mix_refuse(PG_ERR_INVALID, who, "strategy %zu: position column \"%s\" is not a column of the feature store", s, name.c_str());
            if (col->dtype != m->col_dtypes[(size_t)st.pos_decl])
                return mix_refuse(PG_ERR_INVALID, who, "strategy %zu: position column \"%s\" has dtype %d in the feature store, the set was compiled for dtype %d",
                                  s, name.c_str(), col->dtype, m->col_dtypes[(size_t)st.pos_decl]);
            o.pos_col = col->d;
            o.pos_i64 = col->dtype == PG_F_I64;
        }
    }
    if ((rc = m->table.ensure(ctx, who, {{m->pos_table.data(), m->pos_table.size() * 4}}))) return rc;
    a.n_st = (uint32_t)m->st.size();
    a.S = S;
    a.remain = m->remain;
    a.cap = cap;
    a.keep_total = off;
    a.store_rows = fs ? fs->rows : 0;
    a.rows = d_rows;
    a.source = d_source;
    a.order = d_order;
    a.count = d_count;
    a.seed = reinterpret_cast<const unsigned long long*>(d_seed);
    a.user_vals = reinterpret_cast<const unsigned long long*>(d_user_vals);
    a.user_present = d_user_present;
    a.pos_table = m->table.part<int32_t>(0);
    if ((rc = scratch_carve(ctx, kSlotMix, [&](Carve& c) {
            a.mask = c.take<uint8_t>((size_t)nq * cap);
            a.taken = c.take<uint32_t>((size_t)nq * off);
            a.taken_pos = c.take<int32_t>((size_t)nq * off);
        }))) return rc;
    a.out_order = d_out_order;
    a.out_count = d_out_count;
    if (a.n_st) {
        mix_match_kernel<<<dim3((cap + kMixMatchThreads - 1) / kMixMatchThreads, nq), kMixMatchThreads, 0, ctx->stream>>>(p, a);
        PG_HIP(hipGetLastError());
    }
    mix_sort_kernel<<<nq, kMixChunk, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

bool mix_reads_columns(const pg_mix* m) {
    if (m->cond) return true;
    for (const auto& st : m->st)
        if (st.pos_decl >= 0) return true;
    return false;
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_mix_compile(const pg_mix_strategy* strategies, uint32_t n, const pg_cond_col* cols, uint32_t n_cols, uint32_t size, uint32_t remain_item,
                   pg_mix** out) {
    const char* who = "pg_mix_compile";
    PG_REQUIRE(out && (n == 0 || strategies) && (n_cols == 0 || cols), "pg_mix_compile: NULL argument");
    if (n > pg::kMixMaxStrategies) return pg::mix_refuse(PG_ERR_UNSUPPORTED, who, "%u strategies (at most %u)", n, pg::kMixMaxStrategies);
    if (size > pg::kMixMaxSize) return pg::mix_refuse(PG_ERR_UNSUPPORTED, who, "size %u unsupported (at most %u)", size, pg::kMixMaxSize);
    if (n_cols > 256) return pg::mix_refuse(PG_ERR_UNSUPPORTED, who, "%u declared columns (at most 256)", n_cols);
    std::unique_ptr<pg_mix> m(new pg_mix());
    m->size = size;
    m->remain = remain_item ? 1 : 0;
    for (uint32_t d = 0; d < n_cols; ++d) {
        if (!cols[d].name || !cols[d].name[0]) return pg::mix_refuse(PG_ERR_INVALID, who, "declared column %u has no name", d);
        if (cols[d].dtype < PG_F_I32 || cols[d].dtype > PG_F_F64) return pg::mix_refuse(PG_ERR_INVALID, who, "declared column \"%s\" has unknown dtype %d", cols[d].name, cols[d].dtype);
        m->col_names.push_back(cols[d].name);
        m->col_dtypes.push_back(cols[d].dtype);
    }
    std::vector<pg_cond_rule> rules;
    for (uint32_t s = 0; s < n; ++s) {
        const pg_mix_strategy& in = strategies[s];
        pg_mix::Strategy st;
        if (in.type != PG_MIX_FIX && in.type != PG_MIX_RANDOM) return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: unknown strategy type %d", s, in.type);
        st.type = in.type;
        if (in.number < 0) return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: negative number %d", s, in.number);
        if (!(in.number_rate >= 0.0)) return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: negative number_rate %g", s, in.number_rate);
        st.number = (uint32_t)in.number;
        st.rate = in.number_rate;
        st.src_mask = in.source_mask;
        if (in.type == PG_MIX_FIX) {
            if (in.n_positions > pg::kMixMaxPositions)
                return pg::mix_refuse(PG_ERR_UNSUPPORTED, who, "strategy %u: %u positions (at most %u)", s, in.n_positions, pg::kMixMaxPositions);
            if (in.n_positions && !in.positions) return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: NULL positions", s);
            for (uint32_t k = 0; k < in.n_positions; ++k) {
                if (in.positions[k] < 1)
                    return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: position %d (positions count from 1; the reference indexes items[-1])", s, in.positions[k]);
                st.positions.push_back(in.positions[k]);
            }
            st.pos_off = (uint32_t)m->pos_table.size();
            m->pos_table.insert(m->pos_table.end(), st.positions.begin(), st.positions.end());
            if (st.positions.empty() && in.position_field && in.position_field[0]) {
                uint32_t d = 0;
                for (; d < n_cols; ++d)
                    if (!strcmp(cols[d].name, in.position_field)) break;
                if (d == n_cols) return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: position column \"%s\" is not among the declared columns", s, in.position_field);
                if (cols[d].dtype != PG_F_I32 && cols[d].dtype != PG_F_I64)
                    return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: position column \"%s\" is not an int32 / int64 column", s, in.position_field);
                st.pos_decl = (int)d;
            }
        }
        if (in.n_terms) {
            if (!in.terms) return pg::mix_refuse(PG_ERR_INVALID, who, "strategy %u: NULL terms", s);
            st.rule = (uint32_t)rules.size();
            rules.push_back(pg_cond_rule{in.terms, in.n_terms, nullptr});
        }
        m->st.push_back(std::move(st));
    }
    if (!rules.empty()) {
        const int rc = pg_cond_compile(rules.data(), (uint32_t)rules.size(), cols, n_cols, 0, &m->cond);      // (its refusals keep its name; rule r = the r-th strategy with conditions)
        if (rc) return rc;
    }
    *out = m.release();
    return PG_OK;
}

int pg_mix_free(pg_mix* m) {
    if (!m) return PG_OK;
    m->table.release();
    delete m;
    return PG_OK;
}

int pg_mix_num_strategies(const pg_mix* m) { return m ? (int)m->st.size() : 0; }
int pg_mix_num_user_slots(const pg_mix* m) { return m && m->cond ? pg_cond_num_user_slots(m->cond) : 0; }
const char* pg_mix_user_slot_name(const pg_mix* m, int i) { return m && m->cond ? pg_cond_user_slot_name(m->cond, i) : ""; }
int pg_mix_user_slot_is_float(const pg_mix* m, int i) { return m && m->cond ? pg_cond_user_slot_is_float(m->cond, i) : 0; }

int pg_mix_sort_host(const pg_mix* m, uint32_t ctx_size, uint32_t nq, uint32_t cap, const uint8_t* item_in, const void* const* cols,
                     const uint8_t* source, const uint32_t* order, const uint32_t* count, const uint64_t* seed, const uint64_t* user_vals,
                     const uint32_t* user_present, uint32_t* out_order, uint32_t* out_count) {
    const char* who = "pg_mix_sort_host";
    PG_REQUIRE(m && out_order && out_count, "pg_mix_sort_host: NULL argument");
    int rc;
    uint32_t S, number[pg::kMixMaxStrategies] = {0};
    if ((rc = pg::mix_check_call(m, nq, cap, source, user_vals, user_present, who))) return rc;
    if ((rc = pg::mix_numbers(m, ctx_size, who, &S, number))) return rc;
    if (m->cond && (rc = pg::cond_host_check(m->cond, cols, user_vals, who))) return rc;
    for (size_t s = 0; s < m->st.size(); ++s)
        if (m->st[s].pos_decl >= 0 && !(cols && cols[m->st[s].pos_decl]))
            return pg::mix_refuse(PG_ERR_INVALID, who, "the values of position column \"%s\" are missing", m->col_names[(size_t)m->st[s].pos_decl].c_str());
    pg::CondProgram p;
    memset(&p, 0, sizeof p);
    if (m->cond) {
        std::vector<const void*> none(m->cond->col_names.size(), nullptr);
        pg::cond_program(m->cond, none.data(), m->cond->lists.data(), m->cond->progs.data(), 0, &p);
    }
    const size_t ns = m->st.size();
    auto request = [&](uint32_t q, std::vector<uint8_t>& member, std::vector<std::vector<int32_t>>& pos) {
        const size_t q0 = (size_t)q * cap;
        const uint32_t n = count ? std::min(count[q], cap) : cap;
        const uint32_t* ord = order ? order + q0 : nullptr;
        const pg::CondUser u{user_vals ? reinterpret_cast<const unsigned long long*>(user_vals) + (size_t)q * pg::kCondMaxSlots : nullptr,
                             user_present ? user_present[q] : 0u};
        for (size_t s = 0; s < ns; ++s)
            if (m->st[s].pos_decl >= 0) pos[s].assign(n, -1);
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t elem = ord ? ord[j] : j;
            uint32_t bits = 0;
            if (elem < cap) {
                const size_t i = q0 + elem;
                const uint32_t src = source ? source[i] : 0xFFu;
                pg::CondItem it;
                it.item_in = item_in ? item_in[i] != 0 : true;
                if (m->cond) pg::cond_host_item(m->cond->used, m->cond->col_dtypes, cols, item_in, i, &it);
                for (size_t s = 0; s < ns; ++s) {
                    const pg_mix::Strategy& st = m->st[s];
                    bool mem = src < 32u && ((st.src_mask >> src) & 1u) != 0;
                    if (!mem && st.rule != pg::kMixNoRule) mem = pg::cond_rule(p, st.rule, it, u);
                    bits |= mem ? 1u << s : 0u;
                    if (st.pos_decl >= 0 && it.item_in) {
                        const void* col = cols[st.pos_decl];
                        const long long v = m->col_dtypes[(size_t)st.pos_decl] == PG_F_I64 ? ((const long long*)col)[i] : (long long)((const int32_t*)col)[i];
                        pos[s][j] = pg::mix_pos_value(v, S);
                    }
                }
            }
            member[j] = (uint8_t)bits;
        }
        pg::mix_host_request(m, S, number, n, cap, member.data(), pos, ord, seed ? seed[q] : 0ull, out_order + q0, out_count + q);
    };
    // requests are independent: spread over at most 16 threads, request q on thread q mod T (the answer does not depend on T)
    const uint32_t T = std::min<uint32_t>({16u, std::max(1u, std::thread::hardware_concurrency()), nq >= 8 ? nq : 1u});
    auto worker = [&](uint32_t t) {
        std::vector<uint8_t> member(cap);
        std::vector<std::vector<int32_t>> pos(ns);
        for (uint32_t q = t; q < nq; q += T) request(q, member, pos);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < T; ++t) pool.emplace_back(worker, t);
    worker(0);
    for (auto& th : pool) th.join();
    return PG_OK;
}

int pg_mix_sort_dev(pg_ctx* ctx, pg_mix* m, const pg_features* fs, uint32_t ctx_size, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                    const uint8_t* d_source, const uint32_t* d_order, const uint32_t* d_count, const uint64_t* d_seed,
                    const uint64_t* d_user_vals, const uint32_t* d_user_present, uint32_t* d_out_order, uint32_t* d_out_count) {
    const char* who = "pg_mix_sort_dev";
    PG_REQUIRE(ctx && m && d_rows && d_out_order && d_out_count, "pg_mix_sort_dev: NULL argument");
    PG_REQUIRE(fs || !pg::mix_reads_columns(m), "pg_mix_sort_dev: the set reads columns: a feature store is needed");
    int rc;
    uint32_t S, number[pg::kMixMaxStrategies] = {0};
    if ((rc = pg::mix_check_call(m, nq, cap, d_source, d_user_vals, d_user_present, who))) return rc;
    if ((rc = pg::mix_numbers(m, ctx_size, who, &S, number))) return rc;
    PG_REQUIRE(!pg::cand_overlap(d_order, (size_t)nq * cap * 4, d_out_order, (size_t)nq * cap * 4), "pg_mix_sort_dev: d_out_order overlaps d_order");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::mix_sort_locked(ctx, m, fs, S, number, nq, cap, d_rows, d_source, d_order, d_count, d_seed, d_user_vals, d_user_present, d_out_order,
                               d_out_count, who);
}

// ---- one request on host arrays (staged_run, cand_lists.hpp) ---------------------------------------------------------------------
int pg_mix_sort(pg_ctx* ctx, pg_mix* m, const pg_features* fs, uint32_t ctx_size, uint32_t n, const uint64_t* rows, const uint8_t* source,
                const uint32_t* order, uint64_t seed, const uint64_t* user_vals, uint32_t user_present, uint32_t* out_order,
                uint32_t* out_count) {
    const char* who = "pg_mix_sort";
    PG_REQUIRE(ctx && m && out_count && (n == 0 || (rows && out_order)), "pg_mix_sort: NULL argument");
    PG_REQUIRE(fs || !pg::mix_reads_columns(m), "pg_mix_sort: the set reads columns: a feature store is needed");
    if (n == 0) {                                    // an empty request: an empty answer
        *out_count = 0;
        return PG_OK;
    }
    int rc;
    uint32_t S, number[pg::kMixMaxStrategies] = {0};
    if ((rc = pg::mix_check_call(m, 1, n, source, user_vals, &user_present, who))) return rc;
    if ((rc = pg::mix_numbers(m, ctx_size, who, &S, number))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    uint64_t uv[pg::kCondMaxSlots] = {0};
    if (user_vals) memcpy(uv, user_vals, (size_t)pg_mix_num_user_slots(m) * 8);
    using pg::Staged;
    enum { kRows, kUserVals, kSeed, kOrder, kOutOrder, kUserPresent, kCount, kSource };
    Staged st[] = {{rows, (size_t)n * 8, Staged::kIn},
                   {uv, sizeof uv, Staged::kIn},
                   {&seed, 8, Staged::kIn},
                   {order, (size_t)n * 4, Staged::in_if(order)},
                   {out_order, (size_t)n * 4, Staged::kOut},
                   {&user_present, 4, Staged::kIn},
                   {out_count, 4, Staged::kOut},
                   {source, n, Staged::in_if(source)}};
    return pg::staged_run(ctx, pg::kSlotStaging, st, sizeof st / sizeof *st, true /* uv, seed and user_present are this frame's */, [&] {
        return pg::mix_sort_locked(ctx, m, fs, S, number, 1, n, st[kRows].at<uint64_t>(), source ? st[kSource].at<uint8_t>() : nullptr,
                                   order ? st[kOrder].at<uint32_t>() : nullptr, nullptr, st[kSeed].at<uint64_t>(), st[kUserVals].at<uint64_t>(),
                                   st[kUserPresent].at<uint32_t>(), st[kOutOrder].at<uint32_t>(), st[kCount].at<uint32_t>(), who);
    });
}

}  // extern "C"
