// cf_kernel.hpp — the device code that cf.hip (U2I2I, RealTimeU2I's expansion: DESIGN.md 4.1l, 4.1v) and x2i.hip (U2I2X2I: 4.1y)
// run: the keyed fp64 reduction of staged lists in an open-addressed table (cf_accumulate), the sort records and their bitonic
// sort through LDS (cf_finish, cf_sort), the cut and the padding, and the two small kernels of the exclusion path and the
// uploads.  One workgroup of kCfThreads lanes per request.  Included by those two files only; the sort itself is cf_sort.hpp's,
// which hot.hip (list recall: 4.1aa) includes alone.
#pragma once
#include "cf_shared.hpp"
#include "block_rank.hpp"
#include "cf_sort.hpp"

namespace pg {
namespace {

constexpr uint32_t kCfMaxList = 1024;
constexpr uint32_t kCfMaxPairs = 65536;          // a request beyond it is reported, never cut
constexpr uint32_t kCfMaxDepth = 16384;

struct CfArgs {
    const uint64_t* off;
    const uint32_t* nbr;
    const float* sim;
    uint32_t rows;
    uint64_t row_offset;
    const uint32_t* trig;
    const double* pref;
    const uint32_t* trig_off;      // [nq + 1]; NULL: request q's triggers are [q * trig_stride, + min(trig_cnt[q], trig_stride))
    const uint32_t* trig_cnt;      // [nq] (CfTrigDev: what rtu2i.hip's trigger kernel wrote)
    uint32_t trig_stride;
    uint32_t lds_max_pairs;
    uint32_t gslots;               // slots of one request's slice of the global tables (a power of two >= 2 min(65536, rows))
    uint32_t* gkeys;               // [nq][gslots]
    double* gacc;
    ulonglong2* cand;              // [nq][cand_cap] compacted items, then sort records
    uint32_t cand_cap;             // a power of two >= min(65536, rows)
    int normalize;
    uint32_t kd;                   // output depth
    uint64_t* out_rows;            // [nq][kd]
    double* out_scores;
    float* out_idx;                // [nq][kd] or NULL: slot j's own index as bits (the plane pg_exclude_compact_dev carries)
    uint32_t* out_count;           // [nq]
    uint32_t* status;              // the smallest request beyond kCfMaxPairs (UINT32_MAX: none)
};

// what cf_accumulate asks before an entry may claim a slot: cf.hip keeps every entry, x2i.hip drops the request's own triggers
struct CfNoSkip {
    __device__ __forceinline__ bool operator()(uint32_t) const { return false; }
};

// The accumulation over one request's staged triggers and the compaction of its occupied slots into cand[0 .. *n_items), in
// no particular order (the order is made by the sort); *max_bits = the largest positive score's bits.  One body for both
// tiers: keys / acc are LDS or the request's slice of the global tables, `slots` a multiple of kCfThreads.  kMax: the reduction
// of pg_rtu2i_expand — a later term replaces the item's score only when it is larger — in place of the sum.
// skip(item): the entry is dropped before it takes a slot (it never counts towards the maximum either).
template <bool kLds, bool kMax, class Skip = CfNoSkip>
__device__ void cf_accumulate(const CfArgs& a, uint32_t* keys, double* acc, uint32_t slots, uint32_t nt, const uint64_t* tb_begin,
                              const double* tb_pref, const uint32_t* tb_len, ulonglong2* cand, uint32_t* n_items,
                              unsigned long long* max_bits, const Skip& skip = Skip()) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < slots; i += kCfThreads) keys[i] = kCfEmpty;
    // the next trigger's list is loaded while the current one is accumulated
    uint32_t nb_next = kCfEmpty;
    float sm_next = 0.0f;
    if (nt && tid < tb_len[0]) {
        nb_next = a.nbr[tb_begin[0] + tid];
        sm_next = a.sim[tb_begin[0] + tid];
    }
    __syncthreads();
    for (uint32_t j = 0; j < nt; ++j) {
        uint32_t nb = nb_next;
        float sm = sm_next;
        const uint32_t len = tb_len[j];
        const uint64_t begin = tb_begin[j];
        const double pf = tb_pref[j];
        if (j + 1 < nt && tid < tb_len[j + 1]) {
            nb_next = a.nbr[tb_begin[j + 1] + tid];
            sm_next = a.sim[tb_begin[j + 1] + tid];
        }
        for (uint32_t i = tid; i < len; i += kCfThreads) {
            if (i != tid) {                              // (lists are at most kCfThreads long: never taken for an uploaded table)
                nb = a.nbr[begin + i];
                sm = a.sim[begin + i];
            }
            if (nb >= a.rows) continue;
            if (skip(nb)) continue;
            const double term = (double)sm * pf;
            for (uint32_t h = cf_slot(nb, slots);; h = h + 1 == slots ? 0 : h + 1) {
                uint32_t cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                bool mine = false;
                if (cur == kCfEmpty) {
                    cur = atomicCAS(&keys[h], kCfEmpty, nb);
                    mine = cur == kCfEmpty;
                }
                if (mine) {
                    acc[h] = term;                       // the first term of an item IS its score
                    break;
                }
                if (cur == nb) {
                    if (!kMax) acc[h] = acc[h] + term;
                    else if (term > acc[h]) acc[h] = term;
                    break;
                }
            }
        }
        __syncthreads();                                 // trigger j's additions are done, and visible, before trigger j + 1's
    }
    double lmax = 0.0;
    for (uint32_t i = tid; i < slots; i += kCfThreads) {
        const uint32_t key = keys[i];
        const bool occ = key != kCfEmpty;
        const unsigned long long m = __ballot(occ);
        if (m == 0) continue;
        const uint32_t before = ballot_rank(m);
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (occ && before == 0) base = atomicAdd(n_items, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (occ) {
            const double sc = acc[i];
            if (sc > lmax) lmax = sc;
            const uint32_t pos = base + before;
            if (pos < a.cand_cap) cand[pos] = make_ulonglong2((unsigned long long)__double_as_longlong(sc), key);
        }
    }
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const double o = __shfl_xor(lmax, d);
        if (o > lmax) lmax = o;
    }
    // (positive doubles order as their bits)
    if ((tid & (kWave - 1)) == 0 && lmax > 0.0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(lmax));
    __syncthreads();
}

__device__ inline void cf_pad(const CfArgs& a, uint32_t q, uint32_t from) {
    for (uint32_t j = from + threadIdx.x; j < a.kd; j += kCfThreads) {
        const size_t o = (size_t)q * a.kd + j;
        a.out_rows[o] = ~0ull;
        a.out_scores[o] = -__builtin_inf();
        if (a.out_idx) a.out_idx[o] = __uint_as_float(j);
    }
}

// What follows the accumulation of request q: the normalisation, the sort records, their order, the cut and the padding.
// lds: the workgroup's LDS, kCfSortChunk records of it free to order in; *n_items, *max_bits as cf_accumulate left them (not
// inside those bytes).
__device__ void cf_finish(const CfArgs& a, uint32_t q, ulonglong2* cand, const uint32_t* n_items, const unsigned long long* max_bits,
                          unsigned char* lds) {
    const uint32_t tid = threadIdx.x;
    const uint32_t n = min(*n_items, a.cand_cap);
    if (n == 0) {
        if (tid == 0) a.out_count[q] = 0;
        cf_pad(a, q, 0);
        return;
    }
    // m: the largest score, found with > from 0; divided by only when it is positive
    const double m = __longlong_as_double((long long)*max_bits);
    const bool divide = a.normalize && m > 0.0;
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    // sort records: x = the score's bits mapped so that ascending x is descending score (-0.0 ranks as 0.0), y = row << 1 | (the
    // score is -0.0): ascending (x, y) is score descending, then row ascending
    for (uint32_t i = tid; i < np2; i += kCfThreads) {
        ulonglong2 e = make_ulonglong2(~0ull, ~0ull);
        if (i < n) {
            const ulonglong2 c = cand[i];
            double sc = __longlong_as_double((long long)c.x);
            if (divide) sc = sc / m;
            unsigned long long b = (unsigned long long)__double_as_longlong(sc);
            const unsigned long long negzero = b == 0x8000000000000000ull ? 1ull : 0ull;
            if (negzero) b = 0;
            const unsigned long long asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
            e = make_ulonglong2(~asc, (c.y << 1) | negzero);
        }
        cand[i] = e;
    }
    __syncthreads();
    cf_sort(cand, reinterpret_cast<ulonglong2*>(lds), np2);
    const uint32_t kept = min(n, a.kd);
    for (uint32_t j = tid; j < kept; j += kCfThreads) {
        const ulonglong2 e = cand[j];
        const unsigned long long asc = ~e.x;
        unsigned long long b = (asc >> 63) ? (asc & 0x7FFFFFFFFFFFFFFFull) : ~asc;
        if (e.y & 1ull) b = 0x8000000000000000ull;
        const size_t o = (size_t)q * a.kd + j;
        a.out_rows[o] = a.row_offset + (e.y >> 1);
        a.out_scores[o] = __longlong_as_double((long long)b);
        if (a.out_idx) a.out_idx[o] = __uint_as_float(j);
    }
    cf_pad(a, q, kept);
    if (tid == 0) a.out_count[q] = kept;
}

// out[q][j] = scores[q][the index idx[q][j] carries] for the kept slots, -inf behind them
__global__ void cf_gather_scores_kernel(const double* __restrict__ scores, const float* __restrict__ idx, const uint32_t* __restrict__ count,
                                        uint32_t kd, uint32_t k, double* __restrict__ out) {
    const uint32_t q = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    double v = -__builtin_inf();
    if (j < count[q]) {
        const uint32_t src = __float_as_uint(idx[(size_t)q * k + j]);
        if (src < kd) v = scores[(size_t)q * kd + src];
    }
    out[(size_t)q * k + j] = v;
}

__global__ void cf_fill_u64_kernel(uint64_t* __restrict__ p, uint64_t n, uint64_t v) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) p[i] = v;
}

}  // namespace
}  // namespace pg
