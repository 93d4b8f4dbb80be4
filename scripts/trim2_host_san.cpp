// trim2_host_san.cpp — pg_trim2_out_cap and pg_candidates_trim2_host under ASan + UBSan: a stand-alone program
// (scripts/trim2_host_san.sh builds the library's host code with the sanitizers and links this against it).  It runs the host
// statement over the reference tests' three cases (tests/golden/priority_adjust_count_v2.json, merged as UniqueFilter would and
// checked against the answers they pin), over a few hundred generated merges and rule lists — optional arrays present and absent
// (all of them absent among them), padding, all-padding requests, counts up to UINT32_MAX, cap = 1, hostile masks and sources —
// and over every rule list the entry points refuse.  Every call must return a status; nothing may trip a sanitizer.  No device is
// touched.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
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
        std::vector<std::string> recalls, ids;
        for (const auto& r : c.at("recalls").arr) recalls.push_back(r.str);
        auto index_of = [](std::vector<std::string>& v, const std::string& s) {
            auto at = std::find(v.begin(), v.end(), s);
            if (at == v.end()) {
                v.push_back(s);
                return v.size() - 1;
            }
            return (size_t)(at - v.begin());
        };
        // UniqueFilter (filter/unique_filter.go:26-49) on the list: the first item of an id stays, a repeat leaves its score
        std::vector<uint64_t> rows;
        std::vector<double> score, planes;
        std::vector<uint8_t> source;
        std::vector<uint32_t> mask;
        std::map<uint64_t, size_t> at;
        const auto& items = c.at("items").arr;
        const size_t n_planes = recalls.size();
        std::vector<std::vector<double>> pl(n_planes);
        for (const auto& it : items) {
            const uint64_t id = index_of(ids, it.arr[0].str);
            const size_t s = (size_t)(std::find(recalls.begin(), recalls.end(), it.arr[2].str) - recalls.begin());
            const double sc = it.arr[1].num;
            auto seen = at.find(id);
            if (seen == at.end()) {
                at[id] = rows.size();
                rows.push_back(id);
                score.push_back(sc);
                source.push_back((uint8_t)s);
                mask.push_back(1u << s);
                for (size_t p = 0; p < n_planes; ++p) pl[p].push_back(p == s ? sc : 0.0 / 0.0);
            } else {
                mask[seen->second] |= 1u << s;
                pl[s][seen->second] = sc;
            }
        }
        const uint32_t cap = (uint32_t)rows.size();
        for (size_t p = 0; p < n_planes; ++p) planes.insert(planes.end(), pl[p].begin(), pl[p].end());
        std::vector<pg_trim_rule> rules;
        for (const auto& r : c.at("confs").arr)
            rules.push_back(pg_trim_rule{(uint8_t)(std::find(recalls.begin(), recalls.end(), r.s("RecallName")) - recalls.begin()),
                                         (uint8_t)(r.s("Type") == "fix" ? PG_TRIM_FIX : PG_TRIM_ACCUMULATE), (uint32_t)r.d("Count")});
        uint32_t oc = 0, count = 0;
        EXPECT(pg_trim2_out_cap(rules.data(), (uint32_t)rules.size(), cap, &oc) == PG_OK && oc >= 1);
        std::vector<uint64_t> o_rows(oc);
        std::vector<double> o_score(oc), o_planes(n_planes * oc);
        std::vector<uint8_t> o_source(oc);
        std::vector<uint32_t> o_mask(oc);
        EXPECT(pg_candidates_trim2_host(rules.data(), (uint32_t)rules.size(), 1, cap, rows.data(), score.data(), source.data(), nullptr,
                                        planes.data(), (uint32_t)n_planes, mask.data(), nullptr, 0, o_rows.data(), o_score.data(),
                                        o_source.data(), o_planes.data(), o_mask.data(), nullptr, &count) == PG_OK);
        const auto& want_ids = c.at("expect_ids").arr;
        const auto& want_src = c.at("expect_retrieve_ids").arr;
        EXPECT(count == want_ids.size() && count <= oc);
        for (uint32_t j = 0; j < count && j < want_ids.size(); ++j)
            EXPECT(ids[o_rows[j]] == want_ids[j].str && recalls[o_source[j]] == want_src[j].str);
        ++n_cases;
    }
    EXPECT(n_cases == 3);
    return 0;
}

int main(int argc, char** argv) {
    if (golden(argc > 1 ? argv[1] : "tests/golden/priority_adjust_count_v2.json")) return 1;
    const double values[] = {-1.0 / 0.0, -2.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.0, 1.0 / 0.0, 0.0 / 0.0, 5e-324};
    int ok = 0, refused = 0, bare = 0, one = 0, all_pad = 0;
    for (int round = 0; round < 800; ++round) {
        const uint32_t nq = 1 + rnd(3), cap = rnd(8) ? 1 + rnd(90) : 1, n64 = rnd(3) ? 8 : 1 + rnd(8), n32 = 1 + rnd(3);
        const uint32_t n_rules = rnd(25) ? 1 + rnd(5) : rnd(11);
        std::vector<pg_trim_rule> rules(std::max(n_rules, 1u));
        for (uint32_t i = 0; i < rules.size(); ++i) {
            rules[i].source = (uint8_t)(rnd(40) ? (i + round) % 8 : rnd(256));
            rules[i].type = (uint8_t)(rnd(40) ? rnd(2) : rnd(256));
            rules[i].count = rnd(6) ? rnd(2 * cap + 2) : (rnd(2) ? 0xFFFFFFFFu : 0u);
        }
        std::vector<uint64_t> rows((size_t)nq * cap);
        std::vector<double> score(rows.size()), p64((size_t)n64 * rows.size());
        std::vector<uint8_t> source(rows.size());
        std::vector<uint32_t> mask(rows.size()), count(nq);
        std::vector<float> p32((size_t)n32 * rows.size());
        const bool padded = !rnd(12);
        for (size_t i = 0; i < rows.size(); ++i) {
            rows[i] = !padded && rnd(12) ? 1000 + i : ~0ull;
            score[i] = values[rnd(11)];
            source[i] = (uint8_t)(rnd(25) ? rnd(5) : rnd(256));
            mask[i] = rnd(10) ? ((1u << (source[i] & 7)) | (rnd(2) ? 1u << rnd(8) : 0u)) : (uint32_t)g_state;
        }
        for (auto& x : p64) x = values[rnd(11)];
        for (auto& x : p32) x = (float)values[rnd(11)];
        for (auto& x : count) x = rnd(8) ? rnd(cap + 2) : 0xFFFFFFFFu;
        const bool none = !rnd(6);
        const bool w_src = !none && rnd(6), w_cnt = !none && rnd(2), w_p64 = !none && rnd(4), w_mask = !none && rnd(3), w_p32 = !none && rnd(2);
        const uint32_t use_rules = w_src || rnd(4) ? n_rules : std::min(n_rules, 1u);
        uint32_t oc = 0;
        const int rc0 = pg_trim2_out_cap(rules.data(), use_rules, cap, &oc);
        if (rc0 != PG_OK) oc = cap;
        const size_t width = std::max<uint32_t>(oc, 1);                // (every count 0: nothing is written, the outputs still exist)
        std::vector<uint64_t> o_rows((size_t)nq * width);
        std::vector<double> o_score(o_rows.size()), o_p64((size_t)n64 * o_rows.size());
        std::vector<uint8_t> o_source(o_rows.size());
        std::vector<uint32_t> o_mask(o_rows.size()), o_count(nq, 77u);
        std::vector<float> o_p32((size_t)n32 * o_rows.size());
        const int rc = pg_candidates_trim2_host(rules.data(), use_rules, nq, cap, rows.data(), score.data(), w_src ? source.data() : nullptr,
                                                w_cnt ? count.data() : nullptr, w_p64 ? p64.data() : nullptr, n64, w_mask ? mask.data() : nullptr,
                                                w_p32 ? p32.data() : nullptr, n32, o_rows.data(), o_score.data(), w_src ? o_source.data() : nullptr,
                                                w_p64 ? o_p64.data() : nullptr, w_mask ? o_mask.data() : nullptr, w_p32 ? o_p32.data() : nullptr,
                                                o_count.data());
        if (rc == PG_OK) {
            ++ok;
            bare += none;
            one += cap == 1;
            all_pad += padded;
            EXPECT(rc0 == PG_OK);
            for (uint32_t q = 0; q < nq; ++q) {
                EXPECT(o_count[q] <= oc && (!padded || o_count[q] == 0));
                for (uint32_t j = 0; j < oc; ++j) EXPECT((o_rows[(size_t)q * oc + j] == ~0ull) == (j >= o_count[q]));
            }
        } else {
            ++refused;
            EXPECT((rc == PG_ERR_INVALID || rc == PG_ERR_UNSUPPORTED) && std::strlen(pg_last_error()) > 0);
        }
    }
    EXPECT(ok > 300 && refused > 30 && bare > 20 && one > 20 && all_pad > 10);
    std::printf("trim2_host_san: %d served (%d bare, %d of cap 1, %d all padding), %d refused, %d failed checks\n", ok, bare, one, all_pad, refused,
                fails);
    return fails ? 1 : 0;
}
