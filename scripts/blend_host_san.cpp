// blend_host_san.cpp — pg_blend_out_cap and pg_candidates_blend_host under ASan + UBSan: a stand-alone program
// (scripts/blend_host_san.sh builds the library's host code with the sanitizers and links this against it).  It runs the host
// statement over the reference tests' inputs (tests/golden/blend_filters.json, checked against the answers they pin), over a few
// hundred generated merges — every mode, optional arrays present and absent, padding, counts, hostile masks and sources, weights
// up to UINT32_MAX — and over every conf the entry points refuse.  Every call must return a status; nothing may trip a
// sanitizer.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/pairec_gpu.h"
#include "../pairec_amd/host/json.hpp"

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

static int golden(const char* path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    pairec::json::Value root;
    std::string err;
    if (!pairec::json::Parser(ss.str()).Parse(&root, &err)) {
        std::printf("cannot read %s: %s\n", path, err.c_str());
        return 1;
    }
    int n_cases = 0;
    for (const auto& c : root.at("cases").arr) {
        pg_blend_conf conf{};
        const std::string mode = c.s("mode");
        conf.mode = mode == "FAIR" ? PG_BLEND_FAIR : (mode == "SNAKE_SKIP" ? PG_BLEND_SNAKE_SKIP : PG_BLEND_SNAKE_REFILL);
        conf.retain_num = (uint32_t)c.d("retain_num");
        for (const auto& e : c.at("entries").arr) {
            conf.source[conf.n_entries] = (uint8_t)e.arr[0].num;
            conf.weight[conf.n_entries++] = (uint32_t)e.arr[1].num;
        }
        const auto& items = c.at("items").arr;
        const uint32_t cap = (uint32_t)items.size();
        std::vector<uint64_t> rows(cap);
        std::vector<double> score(cap);
        std::vector<uint8_t> source(cap);
        for (uint32_t i = 0; i < cap; ++i) {
            rows[i] = (uint64_t)items[i].arr[0].num;
            score[i] = items[i].arr[1].num;
            source[i] = (uint8_t)items[i].arr[2].num;
        }
        uint32_t oc = 0, count = 0;
        EXPECT(pg_blend_out_cap(&conf, cap, &oc) == PG_OK);
        std::vector<uint64_t> o_rows(oc);
        std::vector<double> o_score(oc);
        std::vector<uint8_t> o_source(oc);
        EXPECT(pg_candidates_blend_host(&conf, 1, cap, rows.data(), score.data(), source.data(), nullptr, nullptr, 0, nullptr, nullptr, 0, o_rows.data(),
                                        o_score.data(), o_source.data(), nullptr, nullptr, nullptr, &count) == PG_OK);
        const auto& ids = c.at("expect_ids").arr;
        const auto& srcs = c.at("expect_sources").arr;
        EXPECT(count == ids.size() && count <= oc);
        for (uint32_t j = 0; j < count && j < ids.size(); ++j) EXPECT(o_rows[j] == (uint64_t)ids[j].num && o_source[j] == (uint8_t)srcs[j].num);
        ++n_cases;
    }
    EXPECT(n_cases >= 6);
    return 0;
}

int main(int argc, char** argv) {
    if (golden(argc > 1 ? argv[1] : "tests/golden/blend_filters.json")) return 1;
    const double values[] = {-1.0 / 0.0, -2.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.0, 1.0 / 0.0, 0.0 / 0.0, 5e-324};
    int ok = 0, refused = 0;
    for (int round = 0; round < 600; ++round) {
        const uint32_t nq = 1 + rnd(3), cap = 1 + rnd(90), n64 = 1 + rnd(8), n32 = 1 + rnd(3);
        pg_blend_conf conf{};
        conf.mode = rnd(40) ? rnd(3) : 3 + rnd(5);
        conf.retain_num = rnd(12) ? 1 + rnd(2 * cap) : (rnd(2) ? 0u : 0xFFFFFFFFu);
        conf.n_entries = rnd(25) ? 1 + rnd(5) : rnd(11);
        for (uint32_t i = 0; i < PG_BLEND_MAX_SOURCES; ++i) {
            conf.source[i] = (uint8_t)(rnd(30) ? (i + round) % 8 : rnd(256));
            conf.weight[i] = rnd(20) ? rnd(6) : (rnd(2) ? 0xFFFFFFFFu : 64u + rnd(3));
        }
        std::vector<uint64_t> rows((size_t)nq * cap);
        std::vector<double> score(rows.size()), p64((size_t)n64 * rows.size());
        std::vector<uint8_t> source(rows.size());
        std::vector<uint32_t> mask(rows.size()), count(nq);
        std::vector<float> p32((size_t)n32 * rows.size());
        for (size_t i = 0; i < rows.size(); ++i) {
            rows[i] = rnd(12) ? 1000 + i : ~0ull;
            score[i] = values[rnd(11)];
            source[i] = (uint8_t)(rnd(25) ? rnd(5) : rnd(256));
            mask[i] = rnd(10) ? ((1u << (source[i] & 7)) | (rnd(2) ? 1u << rnd(8) : 0u)) : (uint32_t)g_state;
        }
        for (auto& x : p64) x = values[rnd(11)];
        for (auto& x : p32) x = (float)values[rnd(11)];
        for (auto& x : count) x = rnd(8) ? rnd(cap + 2) : 0xFFFFFFFFu;
        const bool w_src = rnd(6), w_cnt = rnd(2), w_p64 = rnd(4), w_mask = rnd(3), w_p32 = rnd(2);
        uint32_t oc = 0;
        const int rc0 = pg_blend_out_cap(&conf, cap, &oc);
        if (rc0 != PG_OK) oc = cap;
        std::vector<uint64_t> o_rows((size_t)nq * oc);
        std::vector<double> o_score(o_rows.size()), o_p64((size_t)n64 * o_rows.size());
        std::vector<uint8_t> o_source(o_rows.size());
        std::vector<uint32_t> o_mask(o_rows.size()), o_count(nq);
        std::vector<float> o_p32((size_t)n32 * o_rows.size());
        const int rc = pg_candidates_blend_host(&conf, nq, cap, rows.data(), score.data(), w_src ? source.data() : nullptr, w_cnt ? count.data() : nullptr,
                                                w_p64 ? p64.data() : nullptr, n64, w_mask ? mask.data() : nullptr, w_p32 ? p32.data() : nullptr, n32,
                                                o_rows.data(), o_score.data(), w_src ? o_source.data() : nullptr, w_p64 ? o_p64.data() : nullptr,
                                                w_mask ? o_mask.data() : nullptr, w_p32 ? o_p32.data() : nullptr, o_count.data());
        if (rc == PG_OK) {
            ++ok;
            EXPECT(rc0 == PG_OK);
            for (uint32_t q = 0; q < nq; ++q) {
                EXPECT(o_count[q] <= oc);
                for (uint32_t j = 0; j < oc; ++j) EXPECT((o_rows[(size_t)q * oc + j] == ~0ull) == (j >= o_count[q]));
            }
        } else {
            ++refused;
            EXPECT((rc == PG_ERR_INVALID || rc == PG_ERR_UNSUPPORTED) && std::strlen(pg_last_error()) > 0);
        }
    }
    EXPECT(ok > 150 && refused > 30);
    std::printf("blend_host_san: %d served, %d refused, %d failed checks\n", ok, refused, fails);
    return fails ? 1 : 0;
}
