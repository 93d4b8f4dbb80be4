// fanin.hip — a request's recalls merged on the device: fan-in + UniqueFilter.
//
// RecallService.GetItems (service/recall.go:53-153; the fan-in itself :126-150) runs every recall of the scene's category and
// concatenates what they return; UniqueFilter (filter/unique_filter.go:26-49) then dedups by item id — the first occurrence
// wins and keeps its score (Item.Score) and its recall (RetrieveId), every later occurrence only leaves its score in
// RecallScores[its RetrieveId], overwriting what that recall left before (:43).  Here the recalls' answers already lie in
// device memory as [nq][k_s] rows and scores; one workgroup per request dedups their concatenation in an open-addressed table
// keyed by id, order preserved, without a sort and without leaving the device.
//
// Order-preserving dedup needs more than membership, and nothing here depends on which lane gets anywhere first:
//   insert   every entry claims its id's slot and takes atomicMin(slot value, its position in the concatenation);
//   walk     an entry is a first occurrence iff the slot holds its own position; chunks of kFaninChunk positions in order, first
//            occurrences compacted by block_rank.hpp's chunk_rank and a running base — each leaves its OUTPUT SLOT
//            in the table;
//   planes   per source, every entry takes atomicMax(slot value, (source + 1, index in the source, output slot)) — later sources
//            outrank earlier ones, so nothing is reset — and the entry that finds its own value back is its source's LAST
//            occurrence of the id: it writes the source's plane and mask bit.  What no source wrote is filled with NaN.
//
// Two tiers, chosen per request by the kernel itself: cap <= kFaninLdsMaxCap and ids that span less than 2^32 - 1 keep the
// table in LDS, keyed on the 32-bit distance to the request's smallest id (8 B per slot: 16384 slots = 128 KiB); everything
// else uses the request's slice of context scratch with full 64-bit keys.  Either way two ids that differ anywhere are two ids.
#include "cand_lists.hpp"
#include "block_rank.hpp"

#include <type_traits>

namespace pg {
namespace {

constexpr uint32_t kFaninMaxSources = 8;
constexpr uint32_t kFaninMaxCap = 16384;
constexpr uint32_t kFaninLdsMaxCap = 8192;       // the tier boundary: a larger cap keeps its table in context scratch
constexpr uint32_t kFaninChunk = 1024;           // positions walked at a time = the workgroup's lanes
static_assert(kFaninMaxSources == PG_FANIN_MAX_SOURCES && kFaninMaxCap == PG_FANIN_MAX_CAP && kFaninLdsMaxCap == PG_FANIN_LDS_MAX_CAP &&
                  kFaninChunk == PG_FANIN_CHUNK,
              "include/pairec_gpu.h repeats these");
constexpr uint32_t kFaninThreads = kFaninChunk;
constexpr uint32_t kFaninWaves = kFaninThreads / kWave;
constexpr uint32_t kFaninMinSlots = 1024;        // slots = the power of two >= max(2 cap, this): load factor <= 0.5
constexpr uint32_t kFaninLdsSlots = 2 * kFaninLdsMaxCap;
// LDS tier: keys uint32 [slots] | values uint32 [slots] | mask bytes [cap]; both tiers: wave counts [2][waves], min / max id
constexpr size_t kFaninLdsTable = (size_t)kFaninLdsSlots * 8 + kFaninLdsMaxCap;
constexpr size_t kFaninLds = kFaninLdsTable + 2 * kFaninWaves * 4 + 16;
static_assert(kFaninLds + 256 <= 160 * 1024, "one workgroup's LDS (the source descriptors are static LDS beside it)");
// a slot's value: the smallest position (< 2^14) until the walk, then kFaninSlotFlag | output slot, then
// (source + 1) << 28 | index in the source << 14 | output slot
constexpr uint32_t kFaninSlotFlag = 1u << 14, kFaninSlotMask = kFaninSlotFlag - 1;
static_assert(kFaninMaxCap <= kFaninSlotFlag && kFaninMaxSources + 1 <= 16, "the value's fields");

struct FaninArgs {
    const uint64_t* rows[kFaninMaxSources];
    const void* scores[kFaninMaxSources];
    uint32_t k[kFaninMaxSources];
    uint32_t base[kFaninMaxSources + 1];         // source s holds positions [base[s], base[s + 1])
    uint32_t f64_mask;                           // bit s: source s's scores are fp64
    uint32_t n_src, cap;
    uint32_t slot_bits;                          // log2 of the table's slots, both tiers
    uint32_t lds_max_cap;
    unsigned long long* gkeys;                   // scratch tier: [nq][slots]
    uint32_t* gval;                              // [nq][slots]
    uint32_t* gmask;                             // [nq][cap]
    uint64_t* out_rows;                          // [nq][cap]
    unsigned long long* out_score;               // fp64 bits
    uint8_t* out_source;
    unsigned long long* out_planes;              // [n_src][nq][cap] or NULL
    uint32_t* out_mask;                          // [nq][cap] or NULL
    uint32_t* out_count;                         // [nq]
    uint32_t nq;
};

// float32 bits → the float64 bits of the same value, by integer steps only (no rounding mode, no denormal mode): zeros and
// infinities keep their sign, subnormals become normal, a NaN keeps sign and payload and comes out quiet, as the conversion
// instruction of every host delivers it (vector_recall.go:98 float64(float32))
__device__ inline unsigned long long fanin_widen(uint32_t b) {
    const unsigned long long sign = (unsigned long long)(b >> 31) << 63;
    const uint32_t e = (b >> 23) & 0xFFu;
    uint32_t m = b & 0x7FFFFFu;
    if (e == 0xFFu) return sign | 0x7FF0000000000000ull | ((unsigned long long)m << 29) | (m ? 0x0008000000000000ull : 0ull);
    if (e == 0) {
        if (m == 0) return sign;
        const uint32_t sh = (uint32_t)__clz((int)m) - 8u;                // m * 2^-149 = (m << sh) / 2^23 * 2^(-126 - sh)
        m = (m << sh) & 0x7FFFFFu;
        return sign | ((unsigned long long)(897u - sh) << 52) | ((unsigned long long)m << 29);
    }
    return sign | ((unsigned long long)(e + 896u) << 52) | ((unsigned long long)m << 29);
}

// (exclude.hip's multiplicative hash, scaled to the table: ids that share their low bits spread over it)
__device__ inline uint32_t fanin_slot(unsigned long long key, uint32_t bits) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

// the sources' descriptors, staged in LDS: lanes index them by a position's source
struct FaninDesc {
    const uint64_t* rows[kFaninMaxSources];
    const void* scores[kFaninMaxSources];
    uint32_t k[kFaninMaxSources];
    uint32_t base[kFaninMaxSources + 1];
};

__device__ inline uint32_t fanin_source_of(const FaninDesc& d, uint32_t n_src, uint32_t p) {
    uint32_t s = 0;
    for (uint32_t t = 1; t < n_src; ++t) s += p >= d.base[t] ? 1u : 0u;
    return s;
}

// the slot that holds `key` (it was inserted: the probe ends)
template <bool kLds, typename Key>
__device__ inline uint32_t fanin_find(Key* keys, Key key, uint32_t bits) {
    const uint32_t smask = (1u << bits) - 1u;
    uint32_t h = fanin_slot((unsigned long long)key, bits);
    while (tab_load<kLds>(&keys[h]) != key) h = (h + 1) & smask;
    return h;
}

// One request.  id0: what a key is the distance to (the LDS tier's smallest id; 0 with full keys).  mask: one entry per output
// slot — bytes the source's last occurrence alone touches in LDS, words with atomicOr in scratch.
template <bool kLds>
__device__ void fanin_run(const FaninArgs& a, const FaninDesc& d, uint32_t q, typename std::conditional<kLds, uint32_t, unsigned long long>::type* keys,
                          uint32_t* val, typename std::conditional<kLds, uint8_t, uint32_t>::type* mask, uint32_t* wcnt, unsigned long long id0) {
    typedef typename std::conditional<kLds, uint32_t, unsigned long long>::type Key;
    typedef typename std::conditional<kLds, uint8_t, uint32_t>::type Mask;
    constexpr Key kEmpty = (Key)~(Key)0;         // never a key: the LDS tier's distances are < 2^32 - 1, padding is never inserted
    const uint32_t tid = threadIdx.x;
    const uint32_t bits = a.slot_bits, slots = 1u << bits, smask = slots - 1u, cap = a.cap, n_src = a.n_src;
    const bool want_planes = a.out_planes || a.out_mask;
    for (uint32_t i = tid; i < slots; i += kFaninThreads) {
        tab_store<kLds>(&keys[i], kEmpty);
        tab_store<kLds>(&val[i], ~0u);
    }
    if (want_planes)
        for (uint32_t i = tid; i < cap; i += kFaninThreads) {
            if constexpr (kLds) mask[i] = (Mask)0;
            else tab_store<kLds>(&mask[i], (Mask)0);
        }
    __syncthreads();
    // insert: the id's slot, and the smallest position that holds the id
    for (uint32_t p = tid; p < cap; p += kFaninThreads) {
        const uint32_t s = fanin_source_of(d, n_src, p);
        const unsigned long long id = d.rows[s][(size_t)q * d.k[s] + (p - d.base[s])];
        if (id == kCandPad) continue;
        const Key key = (Key)(id - id0);
        uint32_t h = fanin_slot((unsigned long long)key, bits);
        for (;; h = (h + 1) & smask) {
            // (a read walks the occupied run, the compare-and-swap only claims a slot seen empty: a duplicate finds itself)
            Key cur = tab_load<kLds>(&keys[h]);
            if (cur == kEmpty) cur = atomicCAS(&keys[h], kEmpty, key);
            if (cur == kEmpty || cur == key) break;
        }
        atomicMin(&val[h], p);
    }
    __syncthreads();
    // walk: first occurrences in order
    uint64_t* out_rows = a.out_rows + (size_t)q * cap;
    unsigned long long* out_score = a.out_score + (size_t)q * cap;
    uint8_t* out_source = a.out_source + (size_t)q * cap;
    uint32_t base = 0;
    for (uint32_t c0 = 0, it = 0; c0 < cap; c0 += kFaninChunk, ++it) {
        const uint32_t p = c0 + tid;
        unsigned long long id = kCandPad;
        uint32_t s = 0, j = 0, h = 0;
        bool first = false;
        if (p < cap) {
            s = fanin_source_of(d, n_src, p);
            j = p - d.base[s];
            id = d.rows[s][(size_t)q * d.k[s] + j];
            if (id != kCandPad) {
                h = fanin_find<kLds, Key>(keys, (Key)(id - id0), bits);
                first = tab_load<kLds>(&val[h]) == p;
            }
        }
        uint32_t r, total;
        chunk_rank<kFaninWaves>(first, wcnt, it, &r, &total);
        if (first) {
            const uint32_t dst = base + r;                   // (< cap: at most one first occurrence per position)
            const size_t at = (size_t)q * d.k[s] + j;
            out_rows[dst] = id;
            out_score[dst] = (a.f64_mask >> s) & 1u ? reinterpret_cast<const unsigned long long*>(d.scores[s])[at]
                                                    : fanin_widen(reinterpret_cast<const uint32_t*>(d.scores[s])[at]);
            out_source[dst] = (uint8_t)s;
            // (a later occurrence that reads this instead of the position compares it with its own position: never equal)
            tab_store<kLds>(&val[h], kFaninSlotFlag | dst);
        }
        base += total;
    }
    const uint32_t count = base;
    __syncthreads();
    if (want_planes) {
        // planes: source by source, the last occurrence of every id in the source
        for (uint32_t s = 0; s < n_src; ++s) {
            const uint32_t ks = d.k[s];
            const uint64_t* rows = d.rows[s] + (size_t)q * ks;
            for (uint32_t j = tid; j < ks; j += kFaninThreads) {
                const unsigned long long id = rows[j];
                if (id == kCandPad) continue;
                const uint32_t h = fanin_find<kLds, Key>(keys, (Key)(id - id0), bits);
                // (the value's low bits are the output slot whoever wrote it last)
                const uint32_t slot = tab_load<kLds>(&val[h]) & kFaninSlotMask;
                atomicMax(&val[h], ((s + 1u) << 28) | (j << 14) | slot);
            }
            __syncthreads();
            for (uint32_t j = tid; j < ks; j += kFaninThreads) {
                const unsigned long long id = rows[j];
                if (id == kCandPad) continue;
                const uint32_t h = fanin_find<kLds, Key>(keys, (Key)(id - id0), bits);
                const uint32_t v = tab_load<kLds>(&val[h]);
                if ((v >> 14) != (((s + 1u) << 14) | j)) continue;
                const uint32_t slot = v & kFaninSlotMask;
                if (a.out_planes) {
                    const size_t at = (size_t)q * ks + j;
                    a.out_planes[((size_t)s * a.nq + q) * cap + slot] =
                        (a.f64_mask >> s) & 1u ? reinterpret_cast<const unsigned long long*>(d.scores[s])[at]
                                               : fanin_widen(reinterpret_cast<const uint32_t*>(d.scores[s])[at]);
                }
                // (one lane per output slot and source, a barrier between the sources)
                if constexpr (kLds) mask[slot] = (Mask)(mask[slot] | (1u << s));
                else atomicOr(&mask[slot], 1u << s);
            }
            __syncthreads();                                 // the next source's atomicMax must not reach a slot this one still compares
        }
    }
    // padding behind the distinct ids, the mask, and NaN wherever a source does not hold the slot's item
    for (uint32_t jj = tid; jj < cap; jj += kFaninThreads) {
        if (jj >= count) {
            out_rows[jj] = kCandPad;
            out_score[jj] = kCandNegInf;
            out_source[jj] = 0xFFu;
        }
        if (!want_planes) continue;
        uint32_t mk = 0;
        if (jj < count) {
            if constexpr (kLds) mk = mask[jj];
            else mk = tab_load<kLds>(&mask[jj]);
        }
        if (a.out_mask) a.out_mask[(size_t)q * cap + jj] = mk;
        if (a.out_planes)
            for (uint32_t s = 0; s < n_src; ++s)
                if (!((mk >> s) & 1u)) a.out_planes[((size_t)s * a.nq + q) * cap + jj] = kCandNan;
    }
    if (tid == 0) a.out_count[q] = count;
}

// Request q = blockIdx.x.
__global__ __launch_bounds__(kFaninThreads) void fanin_merge_kernel(FaninArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fanin_lds[];
    __shared__ FaninDesc d;
    uint32_t* wcnt = reinterpret_cast<uint32_t*>(fanin_lds + kFaninLdsTable);
    unsigned long long* mm = reinterpret_cast<unsigned long long*>(wcnt + 2 * kFaninWaves);      // smallest, largest id
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (tid < kFaninMaxSources) {
        d.rows[tid] = a.rows[tid];
        d.scores[tid] = a.scores[tid];
        d.k[tid] = a.k[tid];
    }
    if (tid <= kFaninMaxSources) d.base[tid] = a.base[tid];
    if (tid == 0) {
        mm[0] = ~0ull;
        mm[1] = 0;
    }
    __syncthreads();
    bool lds = a.cap <= a.lds_max_cap;
    unsigned long long id0 = 0;
    if (lds) {
        // the tier is the kernel's own decision, from the request's ids: no host read-back before the launch
        unsigned long long lo = ~0ull, hi = 0;
        for (uint32_t p = tid; p < a.cap; p += kFaninThreads) {
            const uint32_t s = fanin_source_of(d, a.n_src, p);
            const unsigned long long id = d.rows[s][(size_t)q * d.k[s] + (p - d.base[s])];
            if (id == kCandPad) continue;
            lo = id < lo ? id : lo;
            hi = id > hi ? id : hi;
        }
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if ((tid & (kWave - 1)) == 0 && lo <= hi) {
            atomicMin(&mm[0], lo);
            atomicMax(&mm[1], hi);
        }
        __syncthreads();
        lo = mm[0];
        hi = mm[1];
        if (lo <= hi) {
            id0 = lo;
            lds = hi - lo < 0xFFFFFFFFull;
        }
    }
    const uint32_t slots = 1u << a.slot_bits;
    if (lds) {
        uint32_t* keys = reinterpret_cast<uint32_t*>(fanin_lds);
        fanin_run<true>(a, d, q, keys, keys + slots, fanin_lds + (size_t)slots * 8, wcnt, id0);
    } else {
        fanin_run<false>(a, d, q, a.gkeys + (size_t)q * slots, a.gval + (size_t)q * slots, a.gmask + (size_t)q * a.cap, wcnt, 0ull);
    }
}

}  // namespace

// caller holds ctx->mu; one launch on the context's stream, no synchronisation
int fanin_merge_locked(pg_ctx* ctx, const pg_fanin_source* src, uint32_t n_src, uint32_t nq, uint64_t* d_out_rows, double* d_out_score,
                       uint8_t* d_out_source, double* d_out_recall_scores, uint32_t* d_out_source_mask, uint32_t* d_out_count) {
    FaninArgs a{};
    uint32_t cap = 0;
    for (uint32_t s = 0; s < n_src; ++s) {
        a.rows[s] = src[s].d_rows;
        a.scores[s] = src[s].d_scores;
        a.k[s] = src[s].k;
        a.base[s] = cap;
        if (src[s].score_f64) a.f64_mask |= 1u << s;
        cap += src[s].k;
    }
    for (uint32_t s = n_src; s <= kFaninMaxSources; ++s) a.base[s] = cap;
    a.n_src = n_src;
    a.cap = cap;
    a.nq = nq;
    uint32_t bits = 10;
    static_assert((1u << 10) == kFaninMinSlots, "the smallest table");
    while ((1u << bits) < 2 * cap) ++bits;
    a.slot_bits = bits;
    a.lds_max_cap = std::min(ctx->knobs.fanin_lds_max_cap, kFaninLdsMaxCap);
    const size_t slots = (size_t)1 << bits;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotFanin, [&](Carve& c) {
            a.gkeys = c.take<unsigned long long>((size_t)nq * slots);
            a.gval = c.take<uint32_t>((size_t)nq * slots);
            a.gmask = c.take<uint32_t>((size_t)nq * cap);
        }))) return rc;
    a.out_rows = d_out_rows;
    a.out_score = reinterpret_cast<unsigned long long*>(d_out_score);
    a.out_source = d_out_source;
    a.out_planes = reinterpret_cast<unsigned long long*>(d_out_recall_scores);
    a.out_mask = d_out_source_mask;
    a.out_count = d_out_count;
    if ((rc = ensure_dyn_lds(ctx, (const void*)fanin_merge_kernel, kFaninLds))) return rc;
    fanin_merge_kernel<<<nq, kFaninThreads, kFaninLds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_fanin_merge_dev(pg_ctx* ctx, const pg_fanin_source* sources, uint32_t n_sources, uint32_t nq, uint64_t* d_out_rows,
                       double* d_out_score, uint8_t* d_out_source, double* d_out_recall_scores, uint32_t* d_out_source_mask,
                       uint32_t* d_out_count) {
    PG_REQUIRE(ctx && sources && d_out_rows && d_out_score && d_out_source && d_out_count, "pg_fanin_merge_dev: NULL argument");
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)pg::kMaxQueries, "pg_fanin_merge_dev: nq=%u must be in [1,%d]", nq, pg::kMaxQueries);
    if (n_sources < 1 || n_sources > pg::kFaninMaxSources) {
        pg::set_error("pg_fanin_merge_dev: n_sources=%u unsupported (1..%u)", n_sources, pg::kFaninMaxSources);
        return PG_ERR_UNSUPPORTED;
    }
    uint64_t cap = 0;
    for (uint32_t s = 0; s < n_sources; ++s) {
        PG_REQUIRE(sources[s].d_rows && sources[s].d_scores, "pg_fanin_merge_dev: source %u has a NULL list", s);
        if (sources[s].k < 1) {
            pg::set_error("pg_fanin_merge_dev: source %u has k=0 (1 <= k, the sum of all k <= %u)", s, pg::kFaninMaxCap);
            return PG_ERR_UNSUPPORTED;
        }
        cap += sources[s].k;
    }
    if (cap > pg::kFaninMaxCap) {
        pg::set_error("pg_fanin_merge_dev: cap=%llu, the sum of the sources' k, unsupported (<= %u)", (unsigned long long)cap, pg::kFaninMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::fanin_merge_locked(ctx, sources, n_sources, nq, d_out_rows, d_out_score, d_out_source, d_out_recall_scores, d_out_source_mask,
                                  d_out_count);
}

}  // extern "C"
