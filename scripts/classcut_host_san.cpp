// classcut_host_san.cpp — the DiversityAdjustCountFilter front end and host statements under ASan + UBSan: a stand-alone program
// (scripts/classcut_host_san.sh builds the library's host code with the sanitizers and links this against it).  It runs
// pg_classcut_compile, pg_classcut_out_cap, pg_classcut_masks_host and pg_candidates_classcut_host over a fixed table of
// well-formed cases — hostile column values, candidates outside the store, padding, counts, optional arrays present and absent —
// and the compiler over malformed expressions: unterminated quotes, 10 000 nested parentheses, a 1 MB input, an empty string,
// every truncation of a long expression.  Every call must return a status; nothing may trip a sanitizer.  No device is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/pairec_gpu.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return n ? (uint32_t)((g_state >> 11) % n) : 0;
}

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static const pg_cond_col kCols[] = {{"a", PG_F_I32}, {"b", PG_F_I64}, {"c", PG_F_F32}, {"d", PG_F_F64}};
static const char* const kRecalls[] = {"u2i", "hot", "i2i"};

static int compile(const std::vector<pg_classcut_rule>& rules, pg_classcut** out) {
    return pg_classcut_compile(rules.data(), (uint32_t)rules.size(), kCols, 4, kRecalls, 3, out);
}

// one expression that must be refused, with a message
static void refused(const std::string& e) {
    pg_classcut* c = nullptr;
    const int rc = compile({{e.c_str(), PG_TRIM_FIX, 1}}, &c);
    EXPECT(rc == PG_ERR_UNSUPPORTED || rc == PG_ERR_INVALID);
    EXPECT(c == nullptr && pg_last_error()[0] != 0);
    if (c) pg_classcut_free(c);
}

static void malformed() {
    refused("");
    refused("recall_name == 'hot");
    refused("recall_name == \"hot");
    refused("recall_name in ('hot', 'u2i");
    refused("[a");
    refused("a in (1, 2");
    refused(std::string(10000, '(') + "a > 1" + std::string(10000, ')'));
    refused(std::string(10000, '!') + "(a > 1)");
    refused(std::string(10000, '-') + "a > 1");
    std::string big = "a > 1";
    while (big.size() < (1u << 20)) big += " && a > 1";
    refused(big);
    refused(std::string(1u << 20, '('));
    refused(std::string(1u << 20, '\''));
    std::string list = "a in (1";
    for (int i = 0; i < 5000; ++i) list += ", 2";
    refused(list + ")");
    // every truncation of a long well-formed expression either compiles or is refused: never a crash
    const std::string full = "!(a + 1 > b * 2) && (recall_name in ('u2i', \"hot\") || round(d / 3, 1) in (1, -2.5, .5)) || [c] % 2 == -1 ** 2";
    for (size_t n = 0; n <= full.size(); ++n) {
        pg_classcut* c = nullptr;
        const std::string cut = full.substr(0, n);
        const int rc = compile({{cut.c_str(), PG_TRIM_FIX, 1}}, &c);
        EXPECT((rc == PG_OK) == (c != nullptr));
        if (c) pg_classcut_free(c);
    }
    // bytes outside ASCII, control characters
    for (int ch = 1; ch < 256; ++ch) {
        const std::string e = std::string("a > 1 ") + (char)ch + " b";
        pg_classcut* c = nullptr;
        const int rc = compile({{e.c_str(), PG_TRIM_FIX, 1}}, &c);
        EXPECT((rc == PG_OK) == (c != nullptr));
        if (c) pg_classcut_free(c);
    }
    // rule sets the compile refuses
    pg_classcut* c = nullptr;
    EXPECT(pg_classcut_compile(nullptr, 0, kCols, 4, kRecalls, 3, &c) == PG_ERR_INVALID);
    EXPECT(compile({{"a > 1", PG_TRIM_ACCUMULATE, 5}, {"a > 1", PG_TRIM_ACCUMULATE, 4}}, &c) == PG_ERR_INVALID);
    EXPECT(compile({{"a > 1", 7, 5}}, &c) == PG_ERR_INVALID);
    EXPECT(compile({{nullptr, PG_TRIM_FIX, 5}}, &c) == PG_ERR_INVALID);
    EXPECT(compile(std::vector<pg_classcut_rule>(9, pg_classcut_rule{"a > 1", PG_TRIM_FIX, 1}), &c) == PG_ERR_UNSUPPORTED);
    EXPECT(pg_classcut_compile(nullptr, 1, kCols, 4, kRecalls, 3, &c) == PG_ERR_INVALID);
    EXPECT(c == nullptr);
}

static void well_formed() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<std::vector<pg_classcut_rule>> sets = {
        {{"a > 1 || b > 2 && c > 3", PG_TRIM_FIX, 7}},
        {{"recall_name == 'u2i' && a == 3", PG_TRIM_FIX, 4}, {"recall_score > 0.5 || !(b in (1, 2, -3))", PG_TRIM_ACCUMULATE, 9},
         {"recall_name in ('hot', 'nobody')", PG_TRIM_ACCUMULATE, 30}},
        {{"-a ** 2 > 0", PG_TRIM_ACCUMULATE, 0}, {"round(d * 2.5, 1) % 3 <= c / 0", PG_TRIM_FIX, 0xFFFFFFFFu}, {"d == d", PG_TRIM_ACCUMULATE, 0xFFFFFFFFu}},
        {{"recall_score == recall_score", PG_TRIM_FIX, 0}, {"recall_name != \"i2i\"", PG_TRIM_ACCUMULATE, 0}},
        std::vector<pg_classcut_rule>(8, pg_classcut_rule{"a + b + c + d > recall_score", PG_TRIM_FIX, 3}),
    };
    for (const auto& rules : sets) {
        const bool reads_cols = &rules != &sets[3];              // (set 3 reads recall_score and recall_name only: cols may be NULL)
        pg_classcut* c = nullptr;
        EXPECT(compile(rules, &c) == PG_OK && c);
        if (!c) {
            std::printf("%s\n", pg_last_error());
            continue;
        }
        EXPECT(pg_classcut_num_classes(c) == (int)rules.size());
        uint32_t w = 0;
        EXPECT(pg_classcut_out_cap(c, 0, &w) == PG_ERR_UNSUPPORTED && pg_classcut_out_cap(c, PG_TRIM_MAX_CAP + 1, &w) == PG_ERR_UNSUPPORTED);
        for (int round = 0; round < 40; ++round) {
            const uint32_t nq = 1 + rnd(3), cap = 1 + rnd(round < 30 ? 90 : 3000);
            const size_t e = (size_t)nq * cap;
            uint32_t out_cap = 0;
            EXPECT(pg_classcut_out_cap(c, cap, &out_cap) == PG_OK && out_cap <= cap);
            std::vector<int32_t> a(e);
            std::vector<int64_t> b(e);
            std::vector<float> cf(e);
            std::vector<double> d(e), score(e), p64(2 * e);
            std::vector<uint64_t> rows(e);
            std::vector<uint8_t> source(e), item_in(e);
            std::vector<uint32_t> smask(e), count(nq);
            std::vector<float> p32(e);
            const double specials[] = {nan, inf, -inf, -0.0, 0.0, 1e300, -1e300, 5e-324};
            const int64_t bigs[] = {INT64_MIN, INT64_MAX, (1ll << 53) + 1, -(1ll << 53) - 1};
            for (size_t i = 0; i < e; ++i) {
                a[i] = rnd(10) == 0 ? INT32_MIN : (int32_t)rnd(9) - 4;
                b[i] = rnd(8) == 0 ? bigs[rnd(4)] : (int64_t)rnd(9) - 4;
                cf[i] = rnd(6) == 0 ? (float)specials[rnd(8)] : (float)rnd(9) - 4;
                d[i] = rnd(6) == 0 ? specials[rnd(8)] : (double)rnd(9) - 4;
                score[i] = rnd(6) == 0 ? specials[rnd(8)] : (double)rnd(5);
                rows[i] = rnd(12) == 0 ? UINT64_MAX : rnd(100000);
                source[i] = rnd(10) == 0 ? 0xFF : (uint8_t)rnd(5);
                item_in[i] = rnd(5) != 0;
                smask[i] = rnd(16);
                p32[i] = (float)rnd(100);
                p64[i] = p64[e + i] = (double)rnd(100);
            }
            for (uint32_t q = 0; q < nq; ++q) count[q] = rnd(4) == 0 ? cap + rnd(50) : rnd(cap + 1);
            const void* cols[4] = {a.data(), b.data(), cf.data(), d.data()};
            std::vector<uint8_t> masks(e, 0xEE);
            EXPECT(pg_classcut_masks_host(c, (uint32_t)e, round & 1 ? item_in.data() : nullptr, cols, source.data(), score.data(), masks.data()) == PG_OK);
            for (size_t i = 0; i < e; ++i) EXPECT((masks[i] >> rules.size()) == 0);
            const bool opt = (round & 2) != 0;
            std::vector<uint64_t> o_rows(nq * (size_t)out_cap + 1, 7);
            std::vector<double> o_score(nq * (size_t)out_cap + 1, 7), o_p64(2 * nq * (size_t)out_cap + 1, 7);
            std::vector<uint8_t> o_source(nq * (size_t)out_cap + 1, 7);
            std::vector<uint32_t> o_smask(nq * (size_t)out_cap + 1, 7), o_count(nq + 1, 7);
            std::vector<float> o_p32(nq * (size_t)out_cap + 1, 7);
            const int rc = pg_candidates_classcut_host(c, nq, cap, round & 1 ? item_in.data() : nullptr, cols, rows.data(), score.data(), source.data(),
                                                       round & 4 ? count.data() : nullptr, opt ? p64.data() : nullptr, 2, opt ? smask.data() : nullptr,
                                                       opt ? p32.data() : nullptr, 1, o_rows.data(), o_score.data(), o_source.data(),
                                                       opt ? o_p64.data() : nullptr, opt ? o_smask.data() : nullptr, opt ? o_p32.data() : nullptr,
                                                       o_count.data());
            EXPECT(rc == PG_OK);
            EXPECT(o_rows.back() == 7 && o_score.back() == 7 && o_source.back() == 7 && o_count.back() == 7 && o_p64.back() == 7 && o_smask.back() == 7);
            for (uint32_t q = 0; q < nq; ++q) {
                EXPECT(o_count[q] <= out_cap);
                for (uint32_t j = 0; j < out_cap; ++j) EXPECT((o_rows[(size_t)q * out_cap + j] == UINT64_MAX) == (j >= o_count[q]));
            }
            // the calls the host statements refuse
            EXPECT(pg_candidates_classcut_host(c, nq, cap, nullptr, nullptr, rows.data(), score.data(), source.data(), nullptr, nullptr, 0, nullptr, nullptr, 0,
                                               o_rows.data(), o_score.data(), o_source.data(), nullptr, nullptr, nullptr, o_count.data()) ==
                   (reads_cols ? PG_ERR_INVALID : PG_OK));
            EXPECT(pg_candidates_classcut_host(c, nq, cap, nullptr, cols, rows.data(), score.data(), source.data(), nullptr, nullptr, 0, nullptr, nullptr, 0,
                                               o_rows.data(), o_score.data(), nullptr, nullptr, nullptr, nullptr, o_count.data()) == PG_ERR_INVALID);
            EXPECT(pg_candidates_classcut_host(c, 0, cap, nullptr, cols, rows.data(), score.data(), source.data(), nullptr, nullptr, 0, nullptr, nullptr, 0,
                                               o_rows.data(), o_score.data(), o_source.data(), nullptr, nullptr, nullptr, o_count.data()) == PG_ERR_INVALID);
        }
        EXPECT(pg_classcut_free(c) == PG_OK);
    }
    EXPECT(pg_classcut_free(nullptr) == PG_OK);
}

int main() {
    malformed();
    well_formed();
    std::printf(fails ? "classcut_host_san: %d FAILED\n" : "classcut_host_san: all cases ran clean\n", fails);
    return fails ? 1 : 0;
}
