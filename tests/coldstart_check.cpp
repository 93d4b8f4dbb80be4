// A stand-alone check of csrc/coldstart_host.hpp (tests/test_coldstart_san_cpu.py builds it with a host compiler, once plain and
// once under the address and undefined-behaviour sanitizers, and runs it): the OrderBy parser on hostile strings — every prefix
// and every single-byte corruption of the forms it takes, exact-length heap copies so that a read past the terminator is seen —
// and the host statement over the device tests' row counts, pools and depths, checked against what the header promises: ids
// distinct and inside the pool, a permutation at k >= A, the prefix property, the ordered head against a plain sort.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "coldstart_host.hpp"

using namespace pg;

static int g_fail = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);     \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
            if (++g_fail > 20) exit(1);                     \
        }                                                   \
    } while (0)

static uint64_t g_rng = 0x1234567ull;
static uint64_t rnd() { return cold_mix(g_rng += 0x9E3779B97F4A7C15ull); }

// parse an exact-length heap copy; a refusal must name a position inside the text (its end included)
static bool parse(const std::string& s, ColdSpec* spec, size_t* pos) {
    char* p = (char*)malloc(s.size() + 1);
    memcpy(p, s.c_str(), s.size() + 1);
    const char* msg = nullptr;
    *pos = (size_t)-1;
    const bool ok = cold_parse_order(p, spec, pos, &msg);
    if (!ok) CHECK(*pos <= strlen(p) && msg && msg[0], "refusal of \"%s\" names position %zu", s.c_str(), *pos);
    free(p);
    return ok;
}

static void parser_checks() {
    ColdSpec sp;
    size_t pos;
    CHECK(cold_parse_order(nullptr, &sp, &pos, nullptr) && sp.order == kColdRandom, "NULL is the random order");
    const char* forms[] = {"", "random()", " RANDOM ( ) ", "create_time", "create_time desc", "  x_1\tASC\n", "random", "Random Desc"};
    const int orders[] = {kColdRandom, kColdRandom, kColdRandom, kColdAsc, kColdDesc, kColdAsc, kColdAsc, kColdDesc};
    for (size_t f = 0; f < sizeof forms / sizeof *forms; ++f) {
        const std::string s = forms[f];
        CHECK(parse(s, &sp, &pos) && sp.order == orders[f], "\"%s\" parses as order %d", forms[f], orders[f]);
        for (size_t n = 0; n <= s.size(); ++n) (void)parse(s.substr(0, n), &sp, &pos);          // every prefix
        for (size_t i = 0; i < s.size(); ++i)                                                    // every byte, every value but NUL
            for (int c = 1; c < 256; ++c) {
                std::string t = s;
                t[i] = (char)c;
                if (parse(t, &sp, &pos)) CHECK((sp.order == kColdRandom) == sp.column.empty(), "\"%s\": a column exactly when ordered", t.c_str());
            }
    }
    const struct { const char* s; size_t pos; } bad[] = {{"a, b", 1}, {"a + 1", 2}, {"a DESC NULLS FIRST", 7}, {"1a", 0}, {"random(1)", 7},
                                                         {"random(", 7}, {"a b", 2}, {"random() x", 9}, {"(", 0}, {"a desc,", 6}};
    for (const auto& b : bad) CHECK(!parse(b.s, &sp, &pos) && pos == b.pos, "\"%s\" is refused at %zu (got %zu)", b.s, b.pos, pos);
    std::string longname(100000, 'a');
    CHECK(parse(longname + " desc", &sp, &pos) && sp.column.size() == 100000, "a long column name");
    for (int i = 0; i < 2000; ++i) {                                                             // random bytes
        std::string t((size_t)(rnd() % 24), ' ');
        for (char& ch : t) ch = (char)(1 + rnd() % 255);
        (void)parse(t, &sp, &pos);
    }
}

static void key_checks() {
    const double inf = std::numeric_limits<double>::infinity();
    const double vals[] = {-inf, -1e300, -1.5, -4.9e-324, -0.0, 0.0, 4.9e-324, 2.2e-308, 1.5, 1e300, inf};
    for (size_t i = 0; i + 1 < sizeof vals / sizeof *vals; ++i) {
        uint64_t a, b;
        memcpy(&a, &vals[i], 8);
        memcpy(&b, &vals[i + 1], 8);
        const bool zeros = vals[i] == 0.0 && vals[i + 1] == 0.0;
        CHECK(zeros ? cold_key_f64_bits(a) == cold_key_f64_bits(b) : cold_key_f64_bits(a) < cold_key_f64_bits(b), "f64 keys ascend at %zu", i);
        const float fa = (float)vals[i], fb = (float)vals[i + 1];
        uint32_t x, y;
        memcpy(&x, &fa, 4);
        memcpy(&y, &fb, 4);
        CHECK(fa == fb ? cold_key_f32_bits(x) == cold_key_f32_bits(y) : cold_key_f32_bits(x) < cold_key_f32_bits(y), "f32 keys ascend at %zu", i);
    }
    CHECK(cold_key_f64_bits(0x7FF8000000000000ull) == ~0ull && cold_key_f64_bits(0xFFF0000000000001ull) == ~0ull, "every NaN is the largest key");
    CHECK(cold_key_f32_bits(0x7FC00000u) == ~0ull && cold_key_f32_bits(0xFF800001u) == ~0ull, "every NaN is the largest key (f32)");
    CHECK(cold_key_i64(INT64_MIN) == 0 && cold_key_i64(INT64_MAX) == ~0ull && cold_key_i64(-1) < cold_key_i64(0), "integer keys");
}

static void perm_checks() {
    const uint64_t sizes[] = {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 65536, 65537};
    const uint64_t seeds[] = {0, 1, ~0ull, 0x123456789ABCDEF0ull};
    for (uint64_t A : sizes)
        for (uint64_t seed : seeds) {
            const uint32_t h = cold_half_bits(A);
            CHECK((1ull << (2 * h)) >= A && (h == 1 || (1ull << (2 * h - 2)) < A), "half bits of %llu", (unsigned long long)A);
            std::vector<bool> seen(A, false);
            for (uint64_t i = 0; i < A; ++i) {
                const uint64_t p = cold_perm(seed, A, h, i);
                CHECK(p < A && !seen[p], "P is a bijection of [0, %llu)", (unsigned long long)A);
                if (p < A) seen[p] = true;
            }
        }
}

static void statement_checks() {
    const uint64_t row_counts[] = {1, 31, 32, 33, 1023, 1024, 1025, 40000, 300001};
    const uint32_t ks[] = {1, 7, 256, 257, 4096, 16384};
    for (uint64_t rows : row_counts) {
        const size_t words = (size_t)((rows + 31) / 32);
        for (int pool = 0; pool < 7; ++pool) {
            uint32_t* bits = (uint32_t*)calloc(words, 4);                 // exact length: a read past the bitmap is seen
            std::vector<uint32_t> members;
            for (uint64_t r = 0; r < rows; ++r) {
                const bool in = pool == 0 ? false : pool == 1 ? r == 0 : pool == 2 ? r == rows - 1 : pool == 3 ? true : pool == 4 ? r % 3 == 0
                                : pool == 5 ? r >= (rows - 1) / 1024 * 1024 : (r < 1024 || rnd() % 97 == 0);
                if (in) { bits[r >> 5] |= 1u << (r & 31); members.push_back((uint32_t)r); }
            }
            const uint64_t A = members.size();
            const std::set<uint32_t> pool_set(members.begin(), members.end());
            int64_t* col = (int64_t*)malloc(rows * 8);
            for (uint64_t r = 0; r < rows; ++r) col[r] = (int64_t)(rnd() % 5) - 2;          // many ties
            for (uint32_t k : ks) {
                if (rows > 40000 && k != 7 && k != 16384) continue;
                const uint32_t nq = 2, kk = (uint32_t)std::min<uint64_t>(k, A);
                const uint64_t seed[2] = {rnd(), ~0ull};
                std::vector<uint64_t> out((size_t)nq * k);
                std::vector<float> sc((size_t)nq * k);
                uint32_t cnt[2];
                cold_recall_host(kColdRandom, pool == 3 ? nullptr : bits, rows, 5, nullptr, 0, seed, nq, k, out.data(), sc.data(), cnt);
                for (uint32_t q = 0; q < nq; ++q) {
                    std::set<uint64_t> ids;
                    CHECK(cnt[q] == kk, "count");
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint64_t id = out[(size_t)q * k + i];
                        if (i < kk) {
                            CHECK(id >= 5 && pool_set.count((uint32_t)(id - 5)) && ids.insert(id).second && sc[(size_t)q * k + i] == 0.0f,
                                  "rows %llu pool %d k %u: slot %u holds a distinct id of the pool", (unsigned long long)rows, pool, k, i);
                        } else {
                            CHECK(id == ~0ull && sc[(size_t)q * k + i] < 0 && std::isinf(sc[(size_t)q * k + i]), "padding");
                        }
                    }
                    if (k >= A) CHECK(ids.size() == A, "a permutation of the pool at k >= A");
                }
                // ordered, both directions, against a plain sort
                for (int order = kColdAsc; order <= kColdDesc; ++order) {
                    cold_recall_host(order, pool == 3 ? nullptr : bits, rows, 0, col, PG_F_I64, nullptr, nq, k, out.data(), sc.data(), cnt);
                    std::vector<uint32_t> want = members;
                    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return order == kColdAsc ? col[a] < col[b] : col[a] > col[b]; });
                    for (uint32_t q = 0; q < nq; ++q)
                        for (uint32_t i = 0; i < k; ++i)
                            CHECK(out[(size_t)q * k + i] == (i < kk ? want[i] : ~0ull), "rows %llu pool %d k %u order %d slot %u", (unsigned long long)rows,
                                  pool, k, order, i);
                }
            }
            {   // prefix: depth 7 and 256 against 4096 (fresh calls, same seeds)
                const uint64_t seed[2] = {42, ~0ull};
                std::vector<uint64_t> deep(2 * 4096), sh(2 * 256);
                std::vector<float> s1(2 * 4096), s2(2 * 256);
                cold_recall_host(kColdRandom, bits, rows, 0, nullptr, 0, seed, 2, 4096, deep.data(), s1.data(), nullptr);
                for (uint32_t k : {1u, 7u, 256u}) {
                    cold_recall_host(kColdRandom, bits, rows, 0, nullptr, 0, seed, 2, k, sh.data(), s2.data(), nullptr);
                    for (uint32_t q = 0; q < 2; ++q)
                        for (uint32_t i = 0; i < k; ++i) CHECK(sh[(size_t)q * k + i] == deep[(size_t)q * 4096 + i], "prefix at depth %u", k);
                }
            }
            free(col);
            free(bits);
        }
    }
}

int main() {
    parser_checks();
    key_checks();
    perm_checks();
    statement_checks();
    if (g_fail) return 1;
    printf("coldstart OK\n");
    return 0;
}
