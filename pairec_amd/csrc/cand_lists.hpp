// cand_lists.hpp — the candidate lists of nq requests, stated once for the stages that read and write them: the trim (trim.hip),
// the blend (blend.hip), the class cut (classcut.hip), the V2 quota cut (trim2.hip) and ItemStateFilter (cond.hip); the fan-in (fanin.hip), which makes them, takes the constants
// (DESIGN.md 4.1n).
//
// Every array is dense and request-major: an entry is position p < cap of request q, at index q * cap + p; a plane set holds n
// such arrays one behind the other, plane f at f * nq * cap.  The outputs are the same arrays at out_cap.  Real entries lie
// before count[q] (no count: before cap) and have a row other than kCandPad; everything else is padding.
#pragma once
#include "common.hpp"

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

// the ABI's pointers (arguments as pg_candidates_trim_dev) → the two structs: the values as the kernels move them (bits), an
// optional output only where its input is given, no planes counted where the set is NULL
inline void cand_lists_bind(uint32_t nq, uint32_t cap, uint32_t out_cap, const uint64_t* rows, const double* score, const uint8_t* source,
                            const uint32_t* count, const double* planes_f64, uint32_t n_f64, const uint32_t* source_mask,
                            const float* planes_f32, uint32_t n_f32, uint64_t* out_rows, double* out_score, uint8_t* out_source,
                            double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32, uint32_t* out_count, CandIn* in,
                            CandOut* out) {
    in->rows = rows;
    in->score = reinterpret_cast<const unsigned long long*>(score);
    in->source = source;
    in->count = count;
    in->planes64 = reinterpret_cast<const unsigned long long*>(planes_f64);
    in->mask = source_mask;
    in->planes32 = reinterpret_cast<const uint32_t*>(planes_f32);
    in->nq = nq;
    in->cap = cap;
    in->n_f64 = planes_f64 ? n_f64 : 0;
    in->n_f32 = planes_f32 ? n_f32 : 0;
    out->rows = out_rows;
    out->score = reinterpret_cast<unsigned long long*>(out_score);
    out->source = source ? out_source : nullptr;
    out->planes64 = reinterpret_cast<unsigned long long*>(out_planes_f64);
    out->mask = source_mask ? out_source_mask : nullptr;
    out->planes32 = reinterpret_cast<uint32_t*>(out_planes_f32);
    out->count = out_count;
    out->out_cap = out_cap;
}

// what every entry point asks of the optional arrays: an output exactly where its input is given, 1..max_planes planes in a set
inline int cand_lists_check(const char* who, const void* source, const void* planes_f64, uint32_t n_f64, const void* source_mask,
                            const void* planes_f32, uint32_t n_f32, const void* out_source, const void* out_planes_f64,
                            const void* out_source_mask, const void* out_planes_f32, uint32_t max_planes) {
    PG_REQUIRE(!source == !out_source && !source_mask == !out_source_mask, "%s: d_source / d_source_mask and their outputs come in pairs", who);
    PG_REQUIRE(!planes_f64 == !out_planes_f64 && !planes_f32 == !out_planes_f32, "%s: a carried plane set and its output come in pairs", who);
    PG_REQUIRE((!planes_f64 || (n_f64 >= 1 && n_f64 <= max_planes)) && (!planes_f32 || (n_f32 >= 1 && n_f32 <= max_planes)),
               "%s: a carried plane set holds 1..%u planes", who, max_planes);
    return PG_OK;
}

}  // namespace pg
