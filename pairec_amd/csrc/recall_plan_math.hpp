// recall_plan_math.hpp — the arithmetic of the recall plans (recall_plan.hip): how the pilot sample is laid out, which rank seeds
// it, how chunks grow and how large the hit-record areas are.  Pure functions of integers and doubles; the few Knobs values they
// need arrive as arguments.  Plain C++17, no HIP: a host compiler builds this header alone (tests/recall_plan_math_check.cpp),
// at table sizes and K x scale products no test table has.  These values decide launch geometry: the expressions, their double
// arithmetic and their casts are part of the behaviour.
#pragma once
#include <cmath>
#include <cstdint>

namespace pg {

// rows of a block of the table pass (recall.hip), the unit of a table's per-block data (recall_table.hip)
constexpr int kPieceRows = 32;
constexpr uint32_t kCandSlack = 1u << 19;      // candidate capacity beyond K per query
constexpr uint32_t kFirstChunkRows = 32768;
constexpr uint32_t kRecBytes = 48;             // a hit record of the > 128-query int8 screen (recall.hip, at screen_kernel)
constexpr uint32_t kRecPoolSlice = 8192;       // records of the spill pool per decode workgroup
constexpr uint32_t kRecQueries = 256;          // queries of that pass (= kMaxQueries, common.hpp)

inline uint32_t next_pow2(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// The pilot sample of a table of `rows` rows for the best `k`: every stride-th 32-row block, walked in the order
// slot = L * perm_mul mod sample_blocks (scan_kernel's sample_block).  stride < 2: the table has no sample.
struct SampleGeometry {
    uint32_t stride = 1, sample_blocks = 0, k_pilot = 0, perm_mul = 1;
    bool pilot = false;          // the sample holds 4 K' admitted rows: the pilot plan is worth its launches
};
inline SampleGeometry sample_geometry(uint32_t rows, uint32_t k, uint32_t rows_qualified, double pilot_fraction, double pilot_sigmas) {
    SampleGeometry g;
    const uint32_t full_blocks = rows / kPieceRows;           // the sample only uses whole blocks
    // 1/96 of the blocks: with the refinement step of the pilot plan the sample's threshold only serves the
    // first quarter of the full pass, so a thinner, cheaper sample wins (256 requests: 291 vs 286 M items/s at 1/64,
    // 261 M at 1/32; before the refinement 1/64 was best)
    uint32_t want = full_blocks / 96;
    // >= 1M sample rows, but never more than an eighth of the table: small tables are launch-bound, and the pilot's
    // three scan launches beat the growing-chunk plan's nine (1M x 64, K = 200: 0.31 -> 0.13 ms per recall)
    const uint32_t floor_blocks = full_blocks / 8 < 32768 ? full_blocks / 8 : 32768;
    if (want < floor_blocks) want = floor_blocks;
    if (pilot_fraction > 0.0) want = (uint32_t)(full_blocks * pilot_fraction);
    g.stride = want ? full_blocks / want : 1;
    if (g.stride < 2) return g;
    g.sample_blocks = full_blocks / g.stride;
    const double m = (double)k * ((double)g.sample_blocks * kPieceRows / (double)rows);
    g.k_pilot = (uint32_t)ceil(m + pilot_sigmas * sqrt(m) + 8.0);
    // (a filter thins the sample by its selectivity: the sample must still hold 4 K' admitted rows)
    const double admitted = rows ? (double)rows_qualified / (double)rows : 1.0;
    g.pilot = (double)g.k_pilot * 4.0 <= (double)g.sample_blocks * kPieceRows * admitted;
    g.perm_mul = 2654435761u % g.sample_blocks;          // golden-ratio step, made coprime below
    if (g.perm_mul < 2) g.perm_mul = 1;
    auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t r = x % y; x = y; y = r; } return x; };
    while (gcd(g.perm_mul, g.sample_blocks) != 1) ++g.perm_mul;
    return g;
}

// The rank m0 of the seed's score that becomes the threshold of the rest of a screened sample: fewer than K' sample rows
// reaching it has probability < 1e-9 (Poisson tail of the seed's hits among the sample's top K')
inline uint32_t seed_rank(uint32_t seed_rows, uint32_t k_pilot, uint64_t sample_rows) {
    const double mu = (double)seed_rows * (double)k_pilot / (double)sample_rows;
    uint32_t m0 = 1;
    for (double term = exp(-mu), cdf = term; 1.0 - cdf > 1e-9 && m0 < seed_rows; ++m0) {
        term *= mu / (double)m0;          // P(X = m0)
        cdf += term;                      // P(X <= m0)  →  loop ends with P(X >= m0+1) <= 1e-9
    }
    return m0 + 1;
}

// The pilot plan's refinement: the full pass is split after its first quarter (even: the 4-bit screens walk whole 64-row
// pieces) and the thresholds are raised to the k2-th best candidate so far — K' of a sample of a quarter of the table
inline uint32_t refine_split(uint32_t nblocks) { return (nblocks / 4) & ~1u; }
inline uint32_t refine_rank(uint32_t k, double pilot_sigmas) {
    const double m2 = (double)k * 0.25;
    return (uint32_t)ceil(m2 + pilot_sigmas * sqrt(m2) + 8.0);
}

// Blocks of the chunk that starts at logical block `rb` of `nb`, keeping the best `kk`: geometric growth, bounded when `safe`
inline uint32_t next_chunk_blocks(uint32_t rb, uint32_t nb, uint32_t kk, double growth, bool safe) {
    uint32_t chunk_rows;
    if (rb == 0) {
        // every row of the first chunk becomes a candidate of every query: keep it just large
        // enough to seed a meaningful threshold (8 x kk rows, 2048..32768)
        chunk_rows = next_pow2(8 * kk);
        if (chunk_rows < 2048) chunk_rows = 2048;
        if (chunk_rows > kFirstChunkRows || chunk_rows < kk) chunk_rows = kFirstChunkRows;
    } else {
        // chunk = (growth-1) x rows seen: every chunk stages ≈ (growth-1)*kk candidates per query
        const uint64_t grow = (uint64_t)((double)rb * kPieceRows * (growth - 1.0));
        chunk_rows = grow > 0xFFFFFFE0ull ? 0xFFFFFFE0u : (uint32_t)grow;
    }
    if (safe && chunk_rows > kCandSlack / 2) chunk_rows = kCandSlack / 2;
    const uint32_t cb = chunk_rows / kPieceRows;
    return cb > nb - rb ? nb - rb : cb;
}

// The hit-record areas of the > 128-query int8 pass: one region of cap_w records per wave of the launch (8 per CU), then a
// spill pool of pool_cap records, `rec_scale` times their default size (TableLearned::rec_scale_eff)
struct RecordAreas {
    uint32_t floor_w, cap_w, pool_cap;
    uint64_t bytes;              // of the regions and the pool
};
inline RecordAreas record_areas(uint32_t num_cus, uint32_t k, uint32_t rec_scale, uint32_t early_share) {
    RecordAreas r;
    const uint64_t rsc = rec_scale;
    const uint32_t rec_waves = num_cus * 8u;
    // a region per wave: four times the share of 256 x K suspects a wave expects, never below the records the safe
    // plan's bounded chunks can leave in one region
    r.cap_w = (uint32_t)(((uint64_t)kRecQueries * k * 4 * rsc / rec_waves + 255) / 256 * 256);
    // (the safe plan's chunk — kCandSlack / 2 rows — with EVERY row a suspect of every query, e.g. a table in ascending
    //  score order: 16 query blocks of 16 x 64 lanes = 1024 records per block, and the blocks of a SIMD's pair of waves split as screen_kernel splits
    //  them — the larger share decides.  Sized for an even split, the early wave's fifth block went to the spill pool,
    //  which at a small K is small: "overflow in safe mode" on such a table at K = 10, 256 queries.)
    const uint32_t pairs = num_cus * 4u;
    const uint32_t pb = (kCandSlack / 2 / kPieceRows + pairs - 1) / pairs;
    const uint32_t es = early_share > 512 ? early_share : 1024 - early_share;
    uint32_t eb = (uint32_t)(((uint64_t)pb * es + 512) >> 10) + 1;
    if (eb > pb) eb = pb;
    r.floor_w = eb * 1024;
    if (r.cap_w < r.floor_w) r.cap_w = r.floor_w;
    // + a spill pool for tables whose best rows sit together: room for all of 256 x 2 K suspects
    r.pool_cap = (uint32_t)(((uint64_t)kRecQueries * k * 2 * rsc + kRecPoolSlice - 1) / kRecPoolSlice * kRecPoolSlice);
    r.bytes = ((uint64_t)rec_waves * r.cap_w + r.pool_cap) * kRecBytes;
    return r;
}

}  // namespace pg
