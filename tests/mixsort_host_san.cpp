// mixsort_host_san.cpp — a stand-alone program (its own main) that runs MultiRecallMixSort's host side under ASan + UBSan:
// pg_mix_compile / pg_mix_free and pg_mix_sort_host on the reference's test cases (tests/golden/multi_recall_mix_sort.json, argv[1])
// and on a few hundred seeded random configs, refused ones among them.  tests/test_mixsort_san_cpu.py compiles it together with
// csrc/mixsort.hip and csrc/cond.hip — the host code under test, instrumented — and links the rest from the built library.  It
// checks what holds for every answer (the count, no empty slot, no entry twice, every entry of the list, untouched guard words) and
// the facts of the golden cases; the answers themselves are held against tests/mixsort_ref.py by the Python tests.  No GPU is
// touched: nothing here takes a context.
#include "../include/pairec_gpu.h"
#include "../pairec_amd/host/json.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>

namespace json = pairec::json;

static int g_failed = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            ++g_failed;                                         \
        }                                                       \
    } while (0)

static const uint32_t kEmpty = 0xFFFFFFFFu, kGuard = 0xA5A5A5A5u;

struct Strategy {
    int32_t type = PG_MIX_FIX;
    std::vector<int32_t> positions;
    std::string position_field;
    int32_t number = 0;
    double rate = 0.0;
    uint32_t mask = 0;
    std::vector<pg_cond_term> terms;
};

static pg_mix* compile(const std::vector<Strategy>& st, const std::vector<pg_cond_col>& cols, uint32_t size, uint32_t remain, int* rc) {
    std::vector<pg_mix_strategy> in(st.size());
    for (size_t s = 0; s < st.size(); ++s) {
        memset(&in[s], 0, sizeof in[s]);
        in[s].type = st[s].type;
        in[s].positions = st[s].positions.data();
        in[s].n_positions = (uint32_t)st[s].positions.size();
        in[s].position_field = st[s].position_field.c_str();
        in[s].number = st[s].number;
        in[s].number_rate = st[s].rate;
        in[s].source_mask = st[s].mask;
        in[s].terms = st[s].terms.data();
        in[s].n_terms = (uint32_t)st[s].terms.size();
    }
    pg_mix* m = nullptr;
    *rc = pg_mix_compile(in.data(), (uint32_t)in.size(), cols.data(), (uint32_t)cols.size(), size, remain, &m);
    return m;
}

// what holds for every answer of a request of n entries
static void check_answer(const uint32_t* out, uint32_t count, uint32_t n, uint32_t cap, uint32_t S, bool remain, const uint32_t* order, const char* what) {
    const uint32_t want = n < S || remain ? n : S;
    CHECK(count == want, "%s: count %u, expected %u", what, count, want);
    std::vector<uint8_t> in_list(cap, 0), seen(cap, 0);
    for (uint32_t j = 0; j < n; ++j) in_list[order ? order[j] : j] = 1;
    for (uint32_t k = 0; k < cap; ++k) {
        if (k >= count) { CHECK(out[k] == kEmpty, "%s: slot %u behind the count holds %u", what, k, out[k]); continue; }
        CHECK(out[k] < cap && in_list[out[k]] && !seen[out[k]], "%s: slot %u holds %u (empty, foreign or twice)", what, k, out[k]);
        if (out[k] < cap) seen[out[k]] = 1;
    }
}

static pg_cond_term equal_term(const char* name, const char* domain, int type, long long value) {
    pg_cond_term t;
    memset(&t, 0, sizeof t);
    t.name = name;
    t.domain = domain;
    t.op = PG_COND_EQUAL;
    t.type = type;
    t.i = value;
    return t;
}

static void golden(const char* path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    json::Value root;
    std::string err;
    const std::string text = ss.str();
    if (!json::Parser(text).Parse(&root, &err)) { CHECK(false, "golden file %s: %s", path, err.c_str()); return; }
    const json::Value& strings = root.at("strings");
    size_t runs = 0;
    for (const auto& c : root.at("cases").arr) {
        const json::Value& items = c.at("items");
        const uint32_t n = (uint32_t)items.at("source").arr.size();
        std::vector<std::string> recalls;
        for (const auto& r : c.at("recall_names").arr) recalls.push_back(r.str);
        std::vector<uint8_t> source(n);
        std::vector<double> score(n);
        for (uint32_t i = 0; i < n; ++i) { source[i] = (uint8_t)items.at("source").arr[i].num; score[i] = items.at("score").arr[i].num; }
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return score[a] > score[b]; });      // ItemRankScore first
        // the dictionary-coded columns
        std::vector<std::string> col_names;
        std::vector<std::vector<int32_t>> col_vals;
        for (const auto& kv : items.at("columns").obj) {
            col_names.push_back(kv.first);
            col_vals.emplace_back();
            for (const auto& v : kv.second.arr) col_vals.back().push_back((int32_t)v.num);
        }
        std::vector<pg_cond_col> cols(col_names.size());
        std::vector<const void*> col_ptr(col_names.size());
        for (size_t k = 0; k < cols.size(); ++k) { cols[k] = pg_cond_col{col_names[k].c_str(), PG_F_I32}; col_ptr[k] = col_vals[k].data(); }
        std::vector<Strategy> st;
        std::vector<std::string> keep;
        keep.reserve(64);
        for (const auto& r : c.at("config").at("MixSortRules").arr) {
            Strategy s;
            s.type = r.s("MixStrategy") == "fix_position" ? PG_MIX_FIX : PG_MIX_RANDOM;
            for (const auto& p : r.at("Positions").arr) s.positions.push_back((int32_t)p.num);
            s.number = (int32_t)r.n("Number");
            s.rate = r.d("NumberRate");
            for (const auto& name : r.at("RecallNames").arr)
                for (size_t k = 0; k < recalls.size(); ++k)
                    if (recalls[k] == name.str) s.mask |= 1u << k;
            for (const auto& t : r.at("Conditions").arr) {
                keep.push_back(t.s("Name"));
                s.terms.push_back(equal_term(keep.back().c_str(), "item", PG_COND_STRING, strings.n(t.s("Value"))));
            }
            st.push_back(s);
        }
        const bool remain = c.at("config").at("RemainItem").b;
        int rc;
        pg_mix* m = compile(st, cols, (uint32_t)c.at("config").n("Size"), remain, &rc);
        CHECK(rc == PG_OK && m, "%s: compile: %s", c.s("name").c_str(), pg_last_error());
        if (!m) continue;
        for (const auto& sz : c.at("sizes").arr) {
            const uint32_t S = (uint32_t)sz.num;
            std::vector<uint32_t> out(n + 1, kGuard);
            uint32_t count[2] = {kGuard, kGuard};
            const uint64_t seed = S;
            rc = pg_mix_sort_host(m, S, 1, n, nullptr, col_ptr.data(), source.data(), order.data(), nullptr, &seed, nullptr, nullptr, out.data(), count);
            CHECK(rc == PG_OK, "%s size %u: %s", c.s("name").c_str(), S, pg_last_error());
            CHECK(out[n] == kGuard && count[1] == kGuard, "%s size %u: a write behind an output", c.s("name").c_str(), S);
            check_answer(out.data(), count[0], n, n, S, remain, order.data(), c.s("name").c_str());
            const json::Value& facts = c.at("facts");
            if (facts.has("positions_hold") && facts.at("positions_hold").has("scores")) {
                const auto& pos = facts.at("positions_hold").at("positions").arr;
                for (size_t k = 0; k < pos.size(); ++k) {
                    const uint32_t e = out[(size_t)pos[k].num - 1];
                    CHECK(e < n && recalls[source[e]] == facts.at("positions_hold").s("recall_name") && score[e] == facts.at("positions_hold").at("scores").arr[k].num,
                          "%s size %u: position %d holds entry %u", c.s("name").c_str(), S, (int)pos[k].num, e);
                }
            }
            if (facts.has("first_scores"))
                for (size_t k = 0; k < facts.at("first_scores").arr.size(); ++k)
                    CHECK(out[k] < n && score[out[k]] == facts.at("first_scores").arr[k].num, "%s: slot %zu holds score %g", c.s("name").c_str(), k, out[k] < n ? score[out[k]] : -1.0);
            ++runs;
        }
        pg_mix_free(m);
    }
    CHECK(runs == 85, "%zu golden runs, expected 85", runs);
}

static void random_cases() {
    std::mt19937_64 rng(20260101);
    auto below = [&](uint32_t k) { return (uint32_t)(rng() % k); };
    const pg_cond_col cols[2] = {{"c", PG_F_I32}, {"p", PG_F_I64}};
    size_t served = 0, refused = 0;
    for (int iter = 0; iter < 400; ++iter) {
        const uint32_t S = 1 + below(30), nq = 1 + below(4), cap = 1 + below(40);
        const bool remain = below(2) != 0;
        std::vector<Strategy> st(below(5));
        for (auto& s : st) {
            s.type = below(2) ? PG_MIX_FIX : PG_MIX_RANDOM;
            if (s.type == PG_MIX_FIX) {
                const uint32_t k = below(3);
                if (k == 0) for (uint32_t j = 0, e = 1 + below(7); j < e; ++j) s.positions.push_back((int32_t)below(S + 4) + (below(40) ? 1 : 0));   // (rarely 0: refused)
                else if (k == 1) { s.position_field = "p"; s.number = (int32_t)below(42); }
                else s.number = (int32_t)below(6);
            } else if (below(3) == 0) {
                s.rate = 0.1 * below(12);                                   // (above 1: refused at the call)
            } else {
                s.number = (int32_t)below(S + 3) - 1;                       // (-1 and above S: refused)
            }
            s.mask = below(16);
            if (below(2)) s.terms.push_back(equal_term("c", below(2) ? "item" : "", PG_COND_INT, below(4)));
            if (below(6) == 0) s.terms.push_back(equal_term("age", "user", PG_COND_INT, 30));
        }
        int rc;
        pg_mix* m = compile(st, std::vector<pg_cond_col>(cols, cols + 2), below(2) ? S : 0, remain, &rc);
        if (!m) {
            CHECK((rc == PG_ERR_INVALID || rc == PG_ERR_UNSUPPORTED) && pg_last_error()[0], "compile refused with %d", rc);
            ++refused;
            continue;
        }
        const size_t e = (size_t)nq * cap;
        std::vector<int32_t> c(e);
        std::vector<long long> p(e);
        std::vector<uint8_t> source(e), item_in(e);
        std::vector<uint32_t> order(e), count(nq), out(e + 1, kGuard), out_count(nq + 1, kGuard), present(nq);
        std::vector<uint64_t> seed(nq), uv((size_t)nq * PG_COND_MAX_SLOTS, 30);
        for (size_t i = 0; i < e; ++i) { c[i] = (int32_t)below(4); p[i] = (long long)below(S + 6) - 2; source[i] = (uint8_t)below(6); item_in[i] = below(10) != 0; }
        for (uint32_t q = 0; q < nq; ++q) {
            for (uint32_t j = 0; j < cap; ++j) order[(size_t)q * cap + j] = j;
            std::shuffle(order.begin() + (size_t)q * cap, order.begin() + (size_t)(q + 1) * cap, rng);
            count[q] = below(3) ? cap : below(cap + 1);
            seed[q] = rng();
            present[q] = below(2);
        }
        const void* col_ptr[2] = {c.data(), p.data()};
        const bool with_order = below(2) != 0, with_count = below(2) != 0;
        rc = pg_mix_sort_host(m, S, nq, cap, below(2) ? item_in.data() : nullptr, col_ptr, source.data(), with_order ? order.data() : nullptr,
                              with_count ? count.data() : nullptr, below(2) ? seed.data() : nullptr, uv.data(), present.data(), out.data(), out_count.data());
        CHECK(out[e] == kGuard && out_count[nq] == kGuard, "random case %d: a write behind an output", iter);
        if (rc != PG_OK) {
            CHECK(rc == PG_ERR_INVALID && pg_last_error()[0], "random case %d refused with %d", iter, rc);
            ++refused;
        } else {
            for (uint32_t q = 0; q < nq; ++q)
                check_answer(out.data() + (size_t)q * cap, out_count[q], with_count ? std::min(count[q], cap) : cap, cap, S, remain,
                             with_order ? order.data() + (size_t)q * cap : nullptr, "random case");
            ++served;
        }
        pg_mix_free(m);
    }
    CHECK(served >= 200 && refused >= 10, "%zu served, %zu refused", served, refused);
    pg_mix_free(nullptr);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s tests/golden/multi_recall_mix_sort.json\n", argv[0]); return 2; }
    golden(argv[1]);
    random_cases();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("mixsort_host_san OK\n");
    return 0;
}
