// Stand-alone check of pairec_amd/csrc/recall_plan_math.hpp (built and run by test_recall_plan_math_cpu.py; host only).  The
// reference of every function is the expression the recall plans held inline before it moved into the header, restated here
// literally; both are compared over a grid that reaches what no test table can (rows up to 0xFFFFFFE0, K = 16 384 at a record
// scale of 16) and the check stops at the first difference.  Then the properties the launches rely on, and anchors worked out
// from those expressions for 256 CUs, six sigmas and a seed of 8 192 rows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

#include "recall_plan_math.hpp"

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                      \
            std::printf("\n");                                             \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

namespace ref {      // the plans' expressions as recall_job_prepare, recall_job_enqueue and PlanRun had them
constexpr uint32_t kPieceRows = 32, kCandSlack = 1u << 19, kFirstChunkRows = 32768, kRecBytes = 48, kRecPoolSlice = 8192, kMaxQueries = 256;

struct Sample { uint32_t stride, sample_blocks, k_pilot, perm_mul; bool pilot; };
static Sample sample(uint32_t rows, uint32_t k, uint32_t rows_qualified, double pilot_fraction, double pilot_sigmas) {
    Sample j{1, 0, 0, 1, false};
    const uint32_t full_blocks = rows / kPieceRows;
    uint32_t want = full_blocks / 96;
    const uint32_t floor_blocks = full_blocks / 8 < 32768 ? full_blocks / 8 : 32768;
    if (want < floor_blocks) want = floor_blocks;
    if (pilot_fraction > 0.0) want = (uint32_t)(full_blocks * pilot_fraction);
    j.stride = want ? full_blocks / want : 1;
    if (j.stride >= 2) {
        j.sample_blocks = full_blocks / j.stride;
        const double m = (double)k * ((double)j.sample_blocks * kPieceRows / (double)rows);
        j.k_pilot = (uint32_t)ceil(m + pilot_sigmas * sqrt(m) + 8.0);
        const double admitted = rows ? (double)rows_qualified / (double)rows : 1.0;
        if ((double)j.k_pilot * 4.0 <= (double)j.sample_blocks * kPieceRows * admitted) j.pilot = true;
        j.perm_mul = 2654435761u % j.sample_blocks;
        if (j.perm_mul < 2) j.perm_mul = 1;
        auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t r = x % y; x = y; y = r; } return x; };
        while (gcd(j.perm_mul, j.sample_blocks) != 1) ++j.perm_mul;
    }
    return j;
}
static uint32_t m0(uint32_t seed_rows, uint32_t k_pilot, uint64_t sample_rows) {
    const double mu = (double)seed_rows * (double)k_pilot / (double)sample_rows;
    uint32_t m0 = 1;
    for (double term = exp(-mu), cdf = term; 1.0 - cdf > 1e-9 && m0 < seed_rows; ++m0) {
        term *= mu / (double)m0;
        cdf += term;
    }
    ++m0;
    return m0;
}
static uint32_t k2(uint32_t k, double pilot_sigmas) {
    const double m2 = (double)k * 0.25;
    return (uint32_t)ceil(m2 + pilot_sigmas * sqrt(m2) + 8.0);
}
static uint32_t next_pow2(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
static uint32_t chunk_blocks(uint32_t rb, uint32_t nb, uint32_t kk, double growth, bool safe) {
    uint32_t chunk_rows;
    if (rb == 0) {
        chunk_rows = next_pow2(8 * kk);
        if (chunk_rows < 2048) chunk_rows = 2048;
        if (chunk_rows > kFirstChunkRows || chunk_rows < kk) chunk_rows = kFirstChunkRows;
    } else {
        const uint64_t grow = (uint64_t)((double)rb * kPieceRows * (growth - 1.0));
        chunk_rows = grow > 0xFFFFFFE0ull ? 0xFFFFFFE0u : (uint32_t)grow;
    }
    if (safe && chunk_rows > kCandSlack / 2) chunk_rows = kCandSlack / 2;
    uint32_t cb = chunk_rows / kPieceRows;
    if (cb > nb - rb) cb = nb - rb;
    return cb;
}
struct Areas { uint32_t floor_w, cap_w, pool_cap; size_t bytes; };
static Areas areas(int num_cus, uint32_t k, uint32_t rec_scale, uint32_t early_share) {
    const uint32_t rec_waves = (uint32_t)num_cus * 8u;
    const uint64_t rsc = rec_scale;
    uint32_t cap_w = (uint32_t)(((uint64_t)kMaxQueries * k * 4 * rsc / rec_waves + 255) / 256 * 256);
    const uint32_t pairs = (uint32_t)num_cus * 4u;
    const uint32_t pb = (kCandSlack / 2 / kPieceRows + pairs - 1) / pairs;
    const uint32_t es = early_share > 512 ? early_share : 1024 - early_share;
    uint32_t eb = (uint32_t)(((uint64_t)pb * es + 512) >> 10) + 1;
    if (eb > pb) eb = pb;
    const uint32_t floor_w = eb * 1024;
    if (cap_w < floor_w) cap_w = floor_w;
    const uint32_t pool_cap = (uint32_t)(((uint64_t)kMaxQueries * k * 2 * rsc + kRecPoolSlice - 1) / kRecPoolSlice * kRecPoolSlice);
    return {floor_w, cap_w, pool_cap, ((size_t)rec_waves * cap_w + pool_cap) * kRecBytes};
}
}  // namespace ref

static uint32_t gcd(uint32_t x, uint32_t y) { while (y) { const uint32_t r = x % y; x = y; y = r; } return x; }

using Chunks = std::vector<std::pair<uint32_t, uint32_t>>;      // (first block, blocks)
// the schedule grow_scan walks; checks that it tiles [0, nb) and ends
static Chunks schedule(uint32_t nb, uint32_t kk, double growth, bool safe) {
    Chunks out;
    uint32_t rb = 0;
    while (rb < nb) {
        const uint32_t cb = pg::next_chunk_blocks(rb, nb, kk, growth, safe);
        CHECK(cb == ref::chunk_blocks(rb, nb, kk, growth, safe), "chunk at %u of %u, kk %u, growth %g, safe %d", rb, nb, kk, growth, (int)safe);
        CHECK(cb >= 1 && cb <= nb - rb, "a chunk of %u blocks at %u of %u: the loop would not end, or leave the range", cb, rb, nb);
        CHECK(!safe || (uint64_t)cb * 32 <= pg::kCandSlack / 2, "safe chunk of %u blocks", cb);
        out.emplace_back(rb, cb);
        rb += cb;                                                // (next chunk starts where this one ends: no gap, no overlap)
        CHECK(out.size() < (1u << 20), "more than 2^20 chunks over %u blocks", nb);
    }
    CHECK(rb == nb, "schedule ends at %u of %u", rb, nb);
    return out;
}

int main() {
    static_assert(pg::kPieceRows == 32 && pg::kCandSlack == ref::kCandSlack && pg::kFirstChunkRows == ref::kFirstChunkRows &&
                  pg::kRecBytes == ref::kRecBytes && pg::kRecPoolSlice == ref::kRecPoolSlice && pg::kRecQueries == ref::kMaxQueries, "constants");
    static_assert(std::is_same<decltype(pg::RecordAreas::bytes), uint64_t>::value, "the areas' byte size is computed in 64 bits");
    const uint32_t kRows[] = {0u, 31u, 32u, 511u, 4096u, 1000000u, 100000000u, 0xFFFFFFE0u};
    const uint32_t kK[] = {1u, 10u, 200u, 5000u, 16384u};
    const double kSigmas = 6.0;
    const uint32_t kSeed = 8192;
    long compared = 0;

    for (uint32_t rows : kRows)
        for (uint32_t k : kK) {
            for (uint32_t qualified : {rows, rows / 1000, 0u})
                for (double fraction : {0.0, 1.0 / 64})
                    for (double sigmas : {kSigmas, 4.0}) {
                        const pg::SampleGeometry g = pg::sample_geometry(rows, k, qualified, fraction, sigmas);
                        const ref::Sample r = ref::sample(rows, k, qualified, fraction, sigmas);
                        CHECK(g.stride == r.stride && g.sample_blocks == r.sample_blocks && g.k_pilot == r.k_pilot && g.perm_mul == r.perm_mul &&
                                  g.pilot == r.pilot,
                              "sample of %u rows, K %u, %u admitted, fraction %g: stride %u/%u blocks %u/%u K' %u/%u mul %u/%u pilot %d/%d", rows, k,
                              qualified, fraction, g.stride, r.stride, g.sample_blocks, r.sample_blocks, g.k_pilot, r.k_pilot, g.perm_mul, r.perm_mul,
                              (int)g.pilot, (int)r.pilot);
                        ++compared;
                        if (g.stride < 2) {
                            CHECK(g.sample_blocks == 0 && g.k_pilot == 0 && g.perm_mul == 1 && !g.pilot, "a table without a sample has none of its figures");
                            continue;
                        }
                        CHECK(g.sample_blocks >= 1 && (uint64_t)g.sample_blocks * g.stride <= rows / 32, "the sample's blocks lie inside the table");
                        CHECK(g.perm_mul >= 1 && gcd(g.perm_mul, g.sample_blocks) == 1, "perm_mul %u, %u sample blocks", g.perm_mul, g.sample_blocks);
                        const uint64_t sample_rows = (uint64_t)g.sample_blocks * 32;
                        const uint32_t m0 = pg::seed_rank(kSeed, g.k_pilot, sample_rows);
                        CHECK(m0 == ref::m0(kSeed, g.k_pilot, sample_rows), "seed rank, K' %u of %llu sample rows", g.k_pilot, (unsigned long long)sample_rows);
                        CHECK(m0 >= 2 && m0 <= kSeed + 1, "seed rank %u", m0);
                        ++compared;
                    }
            CHECK(pg::refine_rank(k, kSigmas) == ref::k2(k, kSigmas), "k2 of K %u", k);
            const uint32_t nb = (uint32_t)(((uint64_t)rows + 31) / 32);
            CHECK(pg::refine_split(nb) == ((nb / 4) & ~1u), "split of %u blocks", nb);
            for (double growth : {2.0, 4.0, 8.0})
                for (bool safe : {false, true})
                    if (nb >= 1) compared += (long)schedule(nb, k, growth, safe).size();
            for (uint32_t scale : {1u, 2u, 16u})
                for (uint32_t share : {512u, 604u}) {
                    const pg::RecordAreas a = pg::record_areas(256, k, scale, share);
                    const ref::Areas r = ref::areas(256, k, scale, share);
                    CHECK(a.floor_w == r.floor_w && a.cap_w == r.cap_w && a.pool_cap == r.pool_cap && a.bytes == (uint64_t)r.bytes,
                          "record areas, K %u, scale %u, share %u: cap_w %u/%u pool %u/%u", k, scale, share, a.cap_w, r.cap_w, a.pool_cap, r.pool_cap);
                    CHECK(a.cap_w >= a.floor_w && a.cap_w % 256 == 0 && a.floor_w % 256 == 0, "cap_w %u, floor_w %u", a.cap_w, a.floor_w);
                    CHECK(a.pool_cap % pg::kRecPoolSlice == 0 && a.pool_cap >= 2ull * 256 * k * scale, "pool of %u records", a.pool_cap);
                    CHECK(a.bytes == ((uint64_t)2048 * a.cap_w + a.pool_cap) * 48, "bytes");
                    ++compared;
                }
        }

    // ---- anchors (256 CUs, sigmas 6, seed 8 192)
    {
        const pg::SampleGeometry g = pg::sample_geometry(100000000u, 5000, 100000000u, 0.0, kSigmas);
        CHECK(g.stride == 95 && g.sample_blocks == 32894 && g.k_pilot == 105 && g.perm_mul == 21537 && g.pilot, "100 M rows, K 5 000: %u %u %u %u", g.stride,
              g.sample_blocks, g.k_pilot, g.perm_mul);
        CHECK(pg::seed_rank(kSeed, g.k_pilot, (uint64_t)g.sample_blocks * 32) == 13, "100 M rows: m0");
        CHECK(pg::refine_rank(5000, kSigmas) == 1471, "k2 of 5 000");
    }
    {
        const pg::SampleGeometry g = pg::sample_geometry(1000000u, 200, 1000000u, 0.0, kSigmas);
        CHECK(g.stride == 8 && g.sample_blocks == 3906 && g.k_pilot == 63 && g.perm_mul == 187 && g.pilot, "1 M rows, K 200: %u %u %u %u", g.stride,
              g.sample_blocks, g.k_pilot, g.perm_mul);
        CHECK(pg::seed_rank(kSeed, g.k_pilot, (uint64_t)g.sample_blocks * 32) == 23, "1 M rows: m0");
        CHECK(pg::refine_rank(200, kSigmas) == 101, "k2 of 200");
        const pg::SampleGeometry f = pg::sample_geometry(1000000u, 200, 1000u, 0.0, kSigmas);
        CHECK(f.stride == 8 && f.sample_blocks == 3906 && f.k_pilot == 63 && f.perm_mul == 187 && !f.pilot, "1 M rows, 1 000 admitted: no pilot plan");
    }
    {
        const pg::SampleGeometry g = pg::sample_geometry(511u, 1, 511u, 0.0, kSigmas);
        CHECK(g.stride == 15 && g.sample_blocks == 1 && !g.pilot, "511 rows, K 1: %u %u", g.stride, g.sample_blocks);
    }
    {
        const Chunks c = schedule(3125000u, 5000, 2.0, false);
        CHECK(c.size() == 13 && c[0] == std::make_pair(0u, 1024u) && c[1] == std::make_pair(1024u, 1024u) && c[2] == std::make_pair(2048u, 2048u) &&
                  c[3] == std::make_pair(4096u, 4096u) && c[12] == std::make_pair(2097152u, 1027848u),
              "chunks over 3 125 000 blocks, growth 2: %zu", c.size());
        CHECK(schedule(3125000u, 5000, 4.0, true).size() == 383, "chunks over 3 125 000 blocks, growth 4, safe");
        const Chunks d = schedule(31250u, 200, 4.0, false);
        const Chunks want = {{0, 64}, {64, 192}, {256, 768}, {1024, 3072}, {4096, 12288}, {16384, 14866}};
        CHECK(d == want, "chunks over 31 250 blocks, kk 200, growth 4: %zu", d.size());
    }
    {
        const pg::RecordAreas a = pg::record_areas(256, 5000, 1, 604);
        CHECK(a.cap_w == 6144 && a.floor_w == 6144 && a.pool_cap == 2564096 && a.bytes == 727056384ull, "record areas, K 5 000: %u %u %u", a.cap_w, a.floor_w,
              a.pool_cap);
        const pg::RecordAreas b = pg::record_areas(256, 16384, 16, 604);
        CHECK(b.cap_w == 131072 && b.pool_cap == 134217728 && b.bytes == 19327352832ull, "record areas, K 16 384 x 16: %u %u", b.cap_w, b.pool_cap);
    }
    std::printf("recall_plan_math OK (%ld comparisons)\n", compared);
    return 0;
}
