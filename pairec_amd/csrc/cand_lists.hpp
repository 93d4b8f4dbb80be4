// cand_lists.hpp — the candidate lists of nq requests, stated once for the stages that read and write them: the trim (trim.hip),
// the blend (blend.hip), the class cut (classcut.hip), the V2 quota cut (trim2.hip), ItemStateFilter (cond.hip), the value
// cap (dimcap.hip) and the exposure Bloom filter (bloom.hip); the fan-in
// (fanin.hip), which makes them, takes the constants.  Three parts: what the kernels and the host statements
// move (CandIn / CandOut, cand_carry, cand_pad, the sort order and the bit cast); what an entry point is handed (CandCall) and
// the checks every stage runs over it, each in its own order; the staging of a one-request call on host arrays (Staged).
//
// Every array is dense and request-major: an entry is position p < cap of request q, at index q * cap + p; a plane set holds n
// such arrays one behind the other, plane f at f * nq * cap.  The outputs are the same arrays at out_cap.  Real entries lie
// before count[q] (no count: before cap) and have a row other than kCandPad; everything else is padding.
#pragma once
#include "common.hpp"

#include <cstring>

namespace pg {

constexpr uint32_t kCandMaxCap = 16384;
constexpr uint32_t kCandMaxSources = 8;
constexpr uint32_t kCandMaxPlanes = 8;
static_assert(kCandMaxCap == PG_FANIN_MAX_CAP && kCandMaxCap == PG_TRIM_MAX_CAP && kCandMaxCap == PG_BLEND_MAX_CAP &&
                  kCandMaxSources == PG_FANIN_MAX_SOURCES && kCandMaxSources == PG_TRIM_MAX_SOURCES && kCandMaxSources == PG_BLEND_MAX_SOURCES &&
                  kCandMaxPlanes == PG_TRIM_MAX_PLANES && kCandMaxPlanes == PG_BLEND_MAX_PLANES,
              "include/pairec_gpu.h repeats these per stage; the stages are chained, each takes the one before's outputs as they are");
constexpr unsigned long long kCandPad = ~0ull;                       // the row of a padding entry
constexpr unsigned long long kCandNan = 0x7FF8000000000000ull;       // fp64 bits: the quiet NaN
constexpr unsigned long long kCandNegInf = 0xFFF0000000000000ull;    // fp64 bits: -inf

struct CandIn {
    const uint64_t* rows;                        // [nq][cap]
    const unsigned long long* score;             // [nq][cap] fp64 bits
    const uint8_t* source;                       // [nq][cap] or NULL
    const uint32_t* count;                       // [nq] or NULL: every request holds cap entries
    const unsigned long long* planes64;          // [n_f64][nq][cap] fp64 bits or NULL
    const uint32_t* mask;                        // [nq][cap] or NULL
    const uint32_t* planes32;                    // [n_f32][nq][cap] fp32 bits or NULL
    uint32_t nq, cap, n_f64, n_f32;              // (n_f64 / n_f32 = 0 where the plane set is NULL)
};
struct CandOut {
    uint64_t* rows;                              // [nq][out_cap] ...
    unsigned long long* score;
    uint8_t* source;                             // NULL where the input is
    unsigned long long* planes64;
    uint32_t* mask;
    uint32_t* planes32;
    uint32_t* count;                             // [nq]
    uint32_t out_cap;
};

__host__ __device__ __forceinline__ uint32_t cand_n_valid(const CandIn& in, uint32_t q) {
    if (!in.count) return in.cap;
    const uint32_t n = in.count[q];
    return n < in.cap ? n : in.cap;
}

__host__ __device__ __forceinline__ double cand_bits_f64(unsigned long long b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
// pg_sort_scores_dev's order on the host: descending, -0.0 equal to +0.0, NaN last, ties by input position
inline bool cand_before(double x, double y) { return x == x && (y != y || x > y); }
// [a, a + an) and [b, b + bn) share a byte
inline bool cand_overlap(const void* a, size_t an, const void* b, size_t bn) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

// the entry at input index src → output index o (indices into [nq][cap] and [nq][out_cap]): rows, mask and every plane; whole:
// score and source too (the blend writes those two itself: a snake's pick carries the key and the source of the list it came by)
__host__ __device__ __forceinline__ void cand_carry(const CandIn& in, const CandOut& out, size_t src, size_t o, bool whole) {
    out.rows[o] = in.rows[src];
    if (whole) {
        out.score[o] = in.score[src];
        if (out.source) out.source[o] = in.source[src];
    }
    if (out.mask) out.mask[o] = in.mask[src];
    const size_t in_plane = (size_t)in.nq * in.cap, out_plane = (size_t)in.nq * out.out_cap;
    for (uint32_t f = 0; f < in.n_f64; ++f) out.planes64[f * out_plane + o] = in.planes64[f * in_plane + src];
    for (uint32_t f = 0; f < in.n_f32; ++f) out.planes32[f * out_plane + o] = in.planes32[f * in_plane + src];
}

// padding at positions first, first + step, ... < out_cap of request q: row kCandPad, source 0xFF, mask 0, f64 planes NaN, f32
// planes 0.  The score is the one value the stages differ in, so it is the caller's: the trim and the blend pad with -inf
// (kCandNegInf), the Item.Score the fan-in gives its own padding; the filter pads with the quiet NaN (kCandNan), as the planes
// (DESIGN.md 4.1n says why both stay).
__host__ __device__ __forceinline__ void cand_pad(const CandIn& in, const CandOut& out, uint32_t q, uint32_t first, uint32_t step,
                                                  unsigned long long pad_score_bits) {
    const size_t out0 = (size_t)q * out.out_cap, out_plane = (size_t)in.nq * out.out_cap;
    for (uint32_t j = first; j < out.out_cap; j += step) {
        const size_t o = out0 + j;
        out.rows[o] = kCandPad;
        out.score[o] = pad_score_bits;
        if (out.source) out.source[o] = 0xFFu;
        if (out.mask) out.mask[o] = 0u;
        for (uint32_t f = 0; f < in.n_f64; ++f) out.planes64[f * out_plane + o] = kCandNan;
        for (uint32_t f = 0; f < in.n_f32; ++f) out.planes32[f * out_plane + o] = 0u;
    }
}

// Accesses of a per-request open-addressed table that lives in LDS or in context scratch (the fan-in's and the value cap's two
// tiers).  LDS: workgroup scope.  Scratch: every read and write of a slot is an agent-scope atomic, so all of them meet in L2
// whatever the lanes' L1 holds.
template <bool kLds, typename T>
__device__ inline T tab_load(T* p) {
    if constexpr (kLds) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool kLds, typename T>
__device__ inline void tab_store(T* p, T v) {
    if constexpr (kLds) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- an entry point's arguments ---------------------------------------------------------------------------------------------------
// the ABI's list pointers, host or device: pg_candidates_trim_dev's arguments from d_rows on, in its order
struct CandCall {
    const uint64_t* rows;
    const double* score;
    const uint8_t* source;
    const uint32_t* count;
    const double* planes_f64;
    uint32_t n_f64;
    const uint32_t* source_mask;
    const float* planes_f32;
    uint32_t n_f32;
    uint64_t* out_rows;
    double* out_score;
    uint8_t* out_source;
    double* out_planes_f64;
    uint32_t* out_source_mask;
    float* out_planes_f32;
    uint32_t* out_count;
};

// The checks are steps a stage calls in its own order between its own: the first that fails is the call's code and message.
// the pointers no call does without; also: the stage's own (its context, its compiled set)
inline int cand_call_required(const CandCall& l, bool also, const char* who) {
    PG_REQUIRE(also && l.rows && l.score && l.out_rows && l.out_score && l.out_count, "%s: NULL argument", who);
    return PG_OK;
}
inline int cand_check_nq(uint32_t nq, const char* who) {
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    return PG_OK;
}
// the optional arrays: an output exactly where its input is given, 1..max_planes planes in a set
inline int cand_lists_check(const CandCall& l, uint32_t max_planes, const char* who) {
    PG_REQUIRE(!l.source == !l.out_source && !l.source_mask == !l.out_source_mask, "%s: d_source / d_source_mask and their outputs come in pairs", who);
    PG_REQUIRE(!l.planes_f64 == !l.out_planes_f64 && !l.planes_f32 == !l.out_planes_f32, "%s: a carried plane set and its output come in pairs", who);
    PG_REQUIRE((!l.planes_f64 || (l.n_f64 >= 1 && l.n_f64 <= max_planes)) && (!l.planes_f32 || (l.n_f32 >= 1 && l.n_f32 <= max_planes)),
               "%s: a carried plane set holds 1..%u planes", who, max_planes);
    return PG_OK;
}
// no output shares a byte with its input, the inputs at cap, the outputs at out_cap: for the stages whose kernels still read
// a request's inputs after its first output is written (the filter and the two cuts; the trim and the blend do not ask)
inline int cand_call_apart(const CandCall& l, uint32_t nq, uint32_t cap, uint32_t out_cap, const char* who) {
    const size_t e = (size_t)nq * cap, o = (size_t)nq * out_cap;
    PG_REQUIRE(!cand_overlap(l.rows, e * 8, l.out_rows, o * 8) && !cand_overlap(l.score, e * 8, l.out_score, o * 8) &&
                   !cand_overlap(l.source, e, l.out_source, o) && !cand_overlap(l.source_mask, e * 4, l.out_source_mask, o * 4) &&
                   !cand_overlap(l.planes_f64, e * 8 * l.n_f64, l.out_planes_f64, o * 8 * l.n_f64) &&
                   !cand_overlap(l.planes_f32, e * 4 * l.n_f32, l.out_planes_f32, o * 4 * l.n_f32),
               "%s: an output overlaps its input", who);
    return PG_OK;
}
// → the two structs: the values as the kernels move them (bits), an optional output only where its input is given, no planes
// counted where the set is NULL
inline void cand_lists_bind(const CandCall& l, uint32_t nq, uint32_t cap, uint32_t out_cap, CandIn* in, CandOut* out) {
    in->rows = l.rows;
    in->score = reinterpret_cast<const unsigned long long*>(l.score);
    in->source = l.source;
    in->count = l.count;
    in->planes64 = reinterpret_cast<const unsigned long long*>(l.planes_f64);
    in->mask = l.source_mask;
    in->planes32 = reinterpret_cast<const uint32_t*>(l.planes_f32);
    in->nq = nq;
    in->cap = cap;
    in->n_f64 = l.planes_f64 ? l.n_f64 : 0;
    in->n_f32 = l.planes_f32 ? l.n_f32 : 0;
    out->rows = l.out_rows;
    out->score = reinterpret_cast<unsigned long long*>(l.out_score);
    out->source = l.source ? l.out_source : nullptr;
    out->planes64 = reinterpret_cast<unsigned long long*>(l.out_planes_f64);
    out->mask = l.source_mask ? l.out_source_mask : nullptr;
    out->planes32 = reinterpret_cast<uint32_t*>(l.out_planes_f32);
    out->count = l.out_count;
    out->out_cap = out_cap;
}

// ---- one request on host arrays: upload, run, download, synchronise ---------------------------------------------------------------
// A host array of such a call and its place in the scratch slot.  Every array takes its place, in the order given, whether
// this call brings it or not (kSkip: reserved, never copied), so a slot's layout depends on the sizes alone.
struct Staged {
    enum Dir { kIn, kOut, kSkip };
    const void* host;
    size_t bytes;
    Dir dir;
    size_t room;                                 // what it takes of the slot (a call may reserve more than it copies)
    void* dev;                                   // (staged_run's)
    Staged(const void* h, size_t n, Dir d, size_t reserve = 0) : host(h), bytes(n), dir(d), room(reserve ? reserve : n), dev(nullptr) {}
    static Dir in_if(const void* given) { return given ? kIn : kSkip; }
    static Dir out_if(const void* given) { return given ? kOut : kSkip; }
    template <class T>
    T* at() const { return (T*)dev; }
};
// carves the arrays out of `slot`, uploads the kIn ones, runs `launch` (it reads the .dev addresses), downloads the kOut ones into
// their host arrays and synchronises.  sync_uploads: wait for the uploads before `launch`, for a call some of whose sources are
// its own frame's values.  Caller holds ctx->mu.
template <class Launch>
int staged_run(pg_ctx* ctx, ScratchSlot slot, Staged* st, size_t n_st, bool sync_uploads, Launch&& launch) {
    int rc;
    if ((rc = scratch_carve(ctx, slot, [&](Carve& c) {
            for (size_t i = 0; i < n_st; ++i) st[i].dev = c.bytes(st[i].room);
        }))) return rc;
    for (const Staged* s = st; s < st + n_st; ++s)
        if (s->dir == Staged::kIn && s->bytes) PG_HIP(hipMemcpyAsync(s->dev, s->host, s->bytes, hipMemcpyHostToDevice, ctx->stream));
    if (sync_uploads) PG_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = launch())) return rc;
    for (const Staged* s = st; s < st + n_st; ++s)
        if (s->dir == Staged::kOut && s->bytes)
            PG_HIP(hipMemcpyAsync(const_cast<void*>(s->host), s->dev, s->bytes, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

}  // namespace pg
