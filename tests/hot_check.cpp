// hot_check.cpp — csrc/hot_host.hpp alone, built with a host compiler (tests/test_hot_san_cpu.py: plain, and under the address
// and undefined-behaviour sanitizers): the upload validation on hostile offsets and entries (nothing read outside the lists it is
// given), the argument checks, the quota function on zero, tiny and huge values, the draw and the sort key, what a device call stages, and the host statement
// on empty lists, absent triggers and n at its limits against a plain restatement written here.
#include "hot_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <limits>
#include <random>
#include <string>

using namespace pg;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static bool has(const HotRefusal& r, const char* what) { return std::string(r.msg).find(what) != std::string::npos; }

static void check_validate() {
    // exactly-sized heap arrays: a read past a list's end is the sanitizer's to find
    std::vector<uint64_t> off = {2, 4, 4, 5};
    std::vector<uint32_t> rows = {9999, 9999, 1, 2, 3};                    // (the first two entries lie in front of offsets[0]: never read)
    std::vector<double> sc = {std::numeric_limits<double>::quiet_NaN(), 0, 1.0, 0.0, -2.0};
    std::vector<uint8_t> src = {0xFF, 0xFF, 0, 0x80, 126};
    HotRefusal r;
    CHECK(hot_validate_lists("t", 0, 3, off.data(), rows.data(), sc.data(), src.data(), 10, 0, &r));
    CHECK(hot_validate_lists("t", 7, 0, off.data(), nullptr, nullptr, nullptr, 10, 0, &r));              // no triggers: nothing read
    const uint64_t flat[3] = {5, 5, 5};
    CHECK(hot_validate_lists("t", 0, 2, flat, nullptr, nullptr, nullptr, 10, 0, &r));                    // empty lists need no arrays
    CHECK(!hot_validate_lists("t", 0, 3, nullptr, rows.data(), sc.data(), src.data(), 10, 0, &r) && r.code == PG_ERR_INVALID);
    CHECK(!hot_validate_lists("t", 0, 3, off.data(), nullptr, sc.data(), src.data(), 10, 0, &r) && has(r, "NULL"));
    // hostile offsets: descending, wrapping, a list past the limit — refused before any entry is read
    const uint64_t desc[4] = {2, 4, 3, 5}, wrap[3] = {~0ull - 1, 1, 2}, huge[2] = {0, 1ull << 50}, long_[2] = {3, 3 + (uint64_t)kHotMaxEntries + 1};
    CHECK(!hot_validate_lists("t", 0, 3, desc, rows.data(), sc.data(), src.data(), 10, 0, &r) && has(r, "offsets[2] is below offsets[1]"));
    CHECK(!hot_validate_lists("t", 0, 2, wrap, rows.data(), sc.data(), src.data(), 10, 0, &r) && has(r, "is below"));
    CHECK(!hot_validate_lists("t", 4, 1, huge, rows.data(), sc.data(), src.data(), 10, 0, &r) && has(r, "trigger 4 has"));
    CHECK(!hot_validate_lists("t", 0, 1, long_, rows.data(), sc.data(), src.data(), 10, 0, &r) && has(r, "65537 entries"));
    // 2^40 entries in all
    CHECK(!hot_validate_lists("t", 0, 3, off.data(), rows.data(), sc.data(), src.data(), 10, kHotMaxPairs - 3, &r) && has(r, "2^40"));
    CHECK(hot_validate_lists("t", 0, 3, off.data(), rows.data(), sc.data(), src.data(), 10, kHotMaxPairs - 4, &r));
    // entries
    auto bad = [&](int which, size_t at, double v, const char* what) {
        std::vector<uint32_t> r2 = rows;
        std::vector<double> s2 = sc;
        std::vector<uint8_t> b2 = src;
        if (which == 0) r2[at] = (uint32_t)v;
        if (which == 1) s2[at] = v;
        if (which == 2) b2[at] = (uint8_t)v;
        HotRefusal rr;
        CHECK(!hot_validate_lists("t", 0, 3, off.data(), r2.data(), s2.data(), b2.data(), 10, 0, &rr) && rr.code == PG_ERR_INVALID && has(rr, what));
    };
    bad(0, 2, 10, "item row 10 (entry 0 of trigger 0) is outside the table's 10 rows");
    bad(0, 4, 4294967295.0, "entry 0 of trigger 2");
    bad(1, 2, std::numeric_limits<double>::infinity(), "not finite");
    bad(1, 4, std::numeric_limits<double>::quiet_NaN(), "entry 0 of trigger 2 is not finite");
    bad(2, 3, 0xFF, "0xFF");
    bad(1, 3, 5e-324, "marked unscored");
    bad(2, 2, 0x85, "marked unscored");
    // a list of exactly the limit with every row the same is fine
    std::vector<uint64_t> o2 = {0, kHotMaxEntries};
    std::vector<uint32_t> r2(kHotMaxEntries, 7);
    std::vector<double> s2(kHotMaxEntries, 1.0);
    std::vector<uint8_t> b2(kHotMaxEntries, 0);
    CHECK(hot_validate_lists("t", 0, 1, o2.data(), r2.data(), s2.data(), b2.data(), 8, 0, &r));
}

static void check_args() {
    HotRefusal r;
    uint64_t out_r[4] = {0};
    double out_s[4] = {0};
    const uint32_t trig[3] = {0, 1, 2}, off[3] = {0, 1, 3};
    const double val[3] = {1.0, 0.0, 2.0};
    CHECK(hot_check_args("t", PG_HOT_GROUP, trig, nullptr, off, 2, 2, out_r, out_s, &r));
    CHECK(hot_check_args("t", PG_HOT_TOPIC, trig, val, off, 2, 2, out_r, out_s, &r));
    CHECK(!hot_check_args("t", PG_HOT_TOPIC, trig, nullptr, off, 2, 2, out_r, out_s, &r) && has(r, "NULL"));
    CHECK(!hot_check_args("t", PG_HOT_GROUP, nullptr, nullptr, off, 2, 2, out_r, out_s, &r) && has(r, "NULL"));
    const uint32_t none[3] = {4, 4, 4};
    CHECK(hot_check_args("t", PG_HOT_TOPIC, nullptr, nullptr, none, 2, 2, out_r, out_s, &r));           // no triggers: no arrays needed
    CHECK(!hot_check_args("t", 3, trig, val, off, 2, 2, out_r, out_s, &r) && r.code == PG_ERR_INVALID);
    CHECK(!hot_check_args("t", PG_HOT_GROUP, trig, val, off, 0, 2, out_r, out_s, &r) && r.code == PG_ERR_INVALID);
    CHECK(!hot_check_args("t", PG_HOT_GROUP, trig, val, off, 2, 0, out_r, out_s, &r) && r.code == PG_ERR_UNSUPPORTED);
    CHECK(!hot_check_args("t", PG_HOT_GROUP, trig, val, off, 2, kHotMaxK + 1, out_r, out_s, &r) && r.code == PG_ERR_UNSUPPORTED);
    const uint32_t down[3] = {0, 3, 1}, wide[2] = {5, 5 + kHotMaxTriggers + 1}, wrap[2] = {0xFFFFFFF0u, 3};
    CHECK(!hot_check_args("t", PG_HOT_GROUP, trig, val, down, 2, 2, out_r, out_s, &r) && has(r, "is below"));
    CHECK(!hot_check_args("t", PG_HOT_GROUP, trig, val, wide, 1, 2, out_r, out_s, &r) && r.code == PG_ERR_UNSUPPORTED && has(r, "257 triggers"));
    CHECK(!hot_check_args("t", PG_HOT_GROUP, trig, val, wrap, 1, 2, out_r, out_s, &r) && has(r, "is below"));
    for (double v : {-1.0, -5e-324, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
        const double bad[3] = {1.0, 2.0, v};
        CHECK(!hot_check_args("t", PG_HOT_TOPIC, trig, bad, off, 2, 2, out_r, out_s, &r) && r.code == PG_ERR_INVALID &&
              has(r, "trigger 1 of request 1"));
        CHECK(hot_check_args("t", PG_HOT_GLOBAL, trig, bad, off, 2, 2, out_r, out_s, &r));              // read in TOPIC mode only
    }
}

static void check_quotas() {
    uint32_t q[4];
    const double a[2] = {0.0, 1.5};                                        // 0.5 / 1.5 of 2.0: int(2.5), int(7.5)
    hot_topic_quotas(a, 2, 10, q);
    CHECK(q[0] == 2 && q[1] == 7);
    const double zeros[3] = {0.0, 0.0, 0.0};                               // 0.5 each of 1.5: int(3.33), k = 1: 0
    hot_topic_quotas(zeros, 3, 10, q);
    CHECK(q[0] == 3 && q[1] == 3 && q[2] == 3);
    hot_topic_quotas(zeros, 3, 1, q);
    CHECK(q[0] == 0 && q[1] == 0 && q[2] == 0);
    const double one[1] = {5e-324};                                        // a lone subnormal is the whole total
    hot_topic_quotas(one, 1, kHotMaxK, q);
    CHECK(q[0] == kHotMaxK);
    const double tiny[3] = {5e-324, 1.0, 5e-324};
    hot_topic_quotas(tiny, 3, kHotMaxK, q);
    CHECK(q[0] == 0 && q[1] == kHotMaxK && q[2] == 0);
    const double subs[2] = {5e-324, 1.5e-323};                             // 1 and 3 units of the smallest subnormal
    hot_topic_quotas(subs, 2, 8, q);
    CHECK(q[0] == 2 && q[1] == 6);
    const double huge[2] = {1.7e308, 1.7e308};                             // the sum overflows: total = +inf, every share 0
    hot_topic_quotas(huge, 2, kHotMaxK, q);
    CHECK(q[0] == 0 && q[1] == 0);
    const double big[2] = {1.7e308, 1.0};
    hot_topic_quotas(big, 2, 100, q);
    CHECK(q[0] == 100 && q[1] == 0);
    hot_topic_quotas(big, 0, 100, q);                                      // no triggers: nothing written, nothing divided
    CHECK(q[0] == 100);
    const double third[3] = {1.0, 1.0, 1.0};
    hot_topic_quotas(third, 3, 1000, q);
    CHECK(q[0] == 333 && q[1] == 333 && q[2] == 333);
}

static void check_pieces() {
    // splitmix64's first outputs from state 0
    CHECK(hot_draw(0, 0) == (double)(0xE220A8397B1DCDAFull >> 11) * 0x1p-53);
    CHECK(hot_draw(0, 1) == (double)(0x6E789E6AA1B965F4ull >> 11) * 0x1p-53);
    CHECK(hot_draw(0x9E3779B97F4A7C15ull, 0) == hot_draw(0, 1));           // the seed is an offset into one stream
    for (uint32_t p : {0u, 1u, 65535u, 0xFFFFFFFFu}) CHECK(hot_draw(~0ull, p) >= 0.0 && hot_draw(~0ull, p) < 1.0);
    // ascending keys are descending scores; -0.0 ranks as 0.0
    const double order[] = {1.7e308, 16777217.0, 16777216.0, 1.0, 2.2250738585072009e-308, 5e-324, 0.0, -5e-324, -1.0, -1.7e308};
    for (size_t i = 1; i < sizeof order / sizeof *order; ++i) CHECK(hot_key(hot_bits(order[i - 1])) < hot_key(hot_bits(order[i])));
    CHECK(hot_key(hot_bits(-0.0)) == hot_key(hot_bits(0.0)) && hot_bits(-0.0) != hot_bits(0.0));
    CHECK(hot_key(hot_bits(-1.7e308)) < ~0ull);                             // the padding record sorts behind every entry
    CHECK(hot_next_pow2(0) == 1 && hot_next_pow2(1) == 1 && hot_next_pow2(8192) == 8192 && hot_next_pow2(8193) == 16384 &&
          hot_next_pow2(kHotMaxEntries) == kHotMaxEntries);
    CHECK(hot_is_sorted(PG_HOT_GROUP, 0, 5) && !hot_is_sorted(PG_HOT_GLOBAL, 5, 5) && hot_is_sorted(PG_HOT_GLOBAL, 6, 5) &&
          !hot_is_sorted(PG_HOT_TOPIC, 6, 5));
}

// the statement once more, the obvious way: entries collected, stable-sorted by score, cut
static void plain(const HotTableHost& t, int mode, const std::vector<uint32_t>& trig, const std::vector<double>& val, uint64_t seed, uint32_t k,
                  std::vector<uint64_t>* rows, std::vector<uint64_t>* bits, std::vector<uint8_t>* src) {
    std::vector<uint32_t> quota(trig.size() + 1, 0xFFFFFFFFu);
    if (mode == PG_HOT_TOPIC) hot_topic_quotas(val.data(), (uint32_t)trig.size(), k, quota.data());
    struct E { double sc; uint64_t e; };
    std::vector<E> ent;
    for (size_t j = 0; j < trig.size(); ++j) {
        if (trig[j] >= t.n_triggers) continue;
        const uint64_t b = t.offsets[trig[j]], len = std::min<uint64_t>(t.offsets[trig[j] + 1] - b, quota[j]);
        for (uint64_t i = 0; i < len; ++i) {
            const uint64_t e = b + i;
            const uint32_t p = (uint32_t)ent.size();
            ent.push_back({(t.source[e] & 0x80) ? (mode == PG_HOT_GLOBAL ? hot_draw(seed, p) : 0.0) : t.scores[e], e});
        }
    }
    if (mode == PG_HOT_GROUP || (mode == PG_HOT_GLOBAL && ent.size() > k))
        std::stable_sort(ent.begin(), ent.end(), [](const E& a, const E& b) { return a.sc > b.sc; });
    rows->clear();
    bits->clear();
    src->clear();
    for (size_t j = 0; j < ent.size() && j < k; ++j) {
        rows->push_back(t.row_offset + t.item_rows[ent[j].e]);
        bits->push_back(hot_bits(ent[j].sc));
        src->push_back(t.source[ent[j].e] & 0x7F);
    }
}

static void check_statement() {
    std::mt19937_64 rng(11);
    // 12 triggers: empty, one entry, 40000 and 25536 entries (together the limit), 1 more (past it), random ones
    const uint32_t lens[12] = {0, 1, 40000, 25536, 1, 63, 64, 65, 0, 1025, 8193, 300};
    std::vector<uint64_t> off(13, 0);
    for (int i = 0; i < 12; ++i) off[i + 1] = off[i] + lens[i];
    const uint64_t total = off[12];
    const uint64_t rows_n = 70000;
    std::vector<uint32_t> rows(total);
    std::vector<double> sc(total);
    std::vector<uint8_t> src(total);
    const double special[] = {-0.0, 0.0, 5e-324, -5e-324, 1.7e308, -1.7e308, 16777217.0, 16777216.0};
    for (uint64_t e = 0; e < total; ++e) {
        rows[e] = (uint32_t)(rng() % rows_n);
        const uint32_t kind = (uint32_t)(rng() % 8);
        src[e] = (uint8_t)(rng() % 127);
        sc[e] = kind == 0 ? special[rng() % 8] : (double)(rng() % 50);     // many ties
        if (kind == 1) {
            src[e] |= 0x80;
            sc[e] = 0.0;
        }
    }
    HotRefusal r;
    CHECK(hot_validate_lists("t", 0, 12, off.data(), rows.data(), sc.data(), src.data(), rows_n, 0, &r));
    const HotTableHost t{rows_n, 1ull << 33, 12, off.data(), rows.data(), sc.data(), src.data()};
    const std::vector<std::vector<uint32_t>> reqs = {{}, {0}, {0xFFFFFFFFu, 12, 99}, {1}, {2, 3}, {5, 5}, {6, 0xFFFFFFFFu, 7, 8}, {9, 1}, {10}, {11, 10, 11}, {3, 1, 9}};
    for (int mode : {PG_HOT_GROUP, PG_HOT_GLOBAL, PG_HOT_TOPIC})
        for (uint32_t k : {1u, 64u, 300u, 8193u, kHotMaxK}) {
            std::vector<uint32_t> trig, toff = {0};
            std::vector<double> val;
            std::vector<uint64_t> seed;
            for (const auto& rq : reqs) {
                for (uint32_t x : rq) {
                    trig.push_back(x);
                    val.push_back((double)(rng() % 4));                    // zeros among them
                }
                toff.push_back((uint32_t)trig.size());
                seed.push_back(rng());
            }
            const uint32_t nq = (uint32_t)reqs.size();
            std::vector<uint64_t> o_rows((size_t)nq * k);
            std::vector<double> o_sc((size_t)nq * k);
            std::vector<uint8_t> o_src((size_t)nq * k);
            std::vector<uint32_t> o_cnt(nq);
            CHECK(hot_check_args("t", mode, trig.data(), val.data(), toff.data(), nq, k, o_rows.data(), o_sc.data(), &r));
            CHECK(hot_recall_host("t", t, mode, trig.data(), val.data(), toff.data(), seed.data(), nq, k, o_rows.data(), o_sc.data(), o_src.data(),
                                  o_cnt.data(), &r));
            for (uint32_t q = 0; q < nq; ++q) {
                std::vector<uint64_t> w_rows, w_bits;
                std::vector<uint8_t> w_src;
                plain(t, mode, reqs[q], std::vector<double>(val.begin() + toff[q], val.begin() + toff[q + 1]), seed[q], k, &w_rows, &w_bits, &w_src);
                CHECK(o_cnt[q] == w_rows.size());
                bool same = o_cnt[q] == w_rows.size();
                for (uint32_t j = 0; j < k && same; ++j) {
                    const size_t o = (size_t)q * k + j;
                    if (j < w_rows.size()) same = o_rows[o] == w_rows[j] && hot_bits(o_sc[o]) == w_bits[j] && o_src[o] == w_src[j];
                    else same = o_rows[o] == ~0ull && o_sc[o] == -std::numeric_limits<double>::infinity() && o_src[o] == kHotPadSource;
                }
                CHECK(same);
            }
            // the optional outputs and the seeds may be absent
            std::vector<uint64_t> o2((size_t)nq * k);
            std::vector<double> s2((size_t)nq * k);
            CHECK(hot_recall_host("t", t, mode, trig.data(), val.data(), toff.data(), nullptr, nq, k, o2.data(), s2.data(), nullptr, nullptr, &r));
            if (mode != PG_HOT_GLOBAL) CHECK(o2 == o_rows);
        }
    // n at the limit is served, one past it refused by the smallest request's name, nothing written
    const uint32_t trig[] = {2, 3, 2, 3, 4, 2, 3, 1, 4}, toff[] = {0, 2, 5, 9};
    std::vector<uint64_t> o_rows(3 * 4, 123);
    std::vector<double> o_sc(3 * 4, 123.0);
    CHECK(hot_recall_host("t", t, PG_HOT_GROUP, trig, nullptr, toff, nullptr, 1, 4, o_rows.data(), o_sc.data(), nullptr, nullptr, &r));
    std::fill(o_rows.begin(), o_rows.end(), 123);
    CHECK(!hot_recall_host("t", t, PG_HOT_GROUP, trig, nullptr, toff, nullptr, 3, 4, o_rows.data(), o_sc.data(), nullptr, nullptr, &r));
    CHECK(r.code == PG_ERR_UNSUPPORTED && has(r, "request 1 concatenates 65537 entries"));
    CHECK(std::count(o_rows.begin(), o_rows.end(), 123) == 12);
    const double val[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    CHECK(hot_recall_host("t", t, PG_HOT_TOPIC, trig, val, toff, nullptr, 3, 4, o_rows.data(), o_sc.data(), nullptr, nullptr, &r));   // quotas keep n <= k
}

// what a device call stages: every region inside the array (exactly sized: a word past a region's end is the sanitizer's to find),
// the tiers and the slab offsets as the kernel expects them
static void check_stage() {
    const uint32_t lens[6] = {0, 1, 8192, 8193, 40000, 25536};
    std::vector<uint64_t> off(7, 0);
    for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + lens[i];
    HotRefusal r;
    for (int mode : {PG_HOT_GROUP, PG_HOT_GLOBAL, PG_HOT_TOPIC})
        for (uint32_t nq : {1u, 2u, 7u, kHotMaxQueries}) {
            std::vector<uint32_t> trig, toff = {0};
            std::vector<double> val;
            const std::vector<std::vector<uint32_t>> kinds = {{}, {1}, {2}, {3, 0xFFFFFFFFu}, {4, 5}, {3, 2, 1}, std::vector<uint32_t>(kHotMaxTriggers, 1)};
            for (uint32_t q = 0; q < nq; ++q) {
                for (uint32_t x : kinds[(q + nq) % kinds.size()]) {
                    trig.push_back(x);
                    val.push_back(1.0 + x);
                }
                toff.push_back((uint32_t)trig.size());
            }
            // offsets that do not start at 0: the staged ones do
            for (auto& x : toff) x += 5;
            trig.insert(trig.begin(), 5, 77u);
            val.insert(val.begin(), 5, -1.0);
            const uint32_t k = 8192, total = toff[nq] - toff[0];
            HotStage st;
            CHECK(hot_stage_build("t", mode, 6, off.data(), trig.data(), val.data(), toff.data(), nq, k, &st, &r));
            CHECK(st.n_at == nq + 1 && st.slab_at == 2 * (size_t)nq + 1 && st.trig_at == 3 * (size_t)nq + 1 && st.quota_at == st.trig_at + total);
            CHECK(st.words.size() == st.quota_at + (mode == PG_HOT_TOPIC ? total : 0));
            size_t slab = 0;
            uint32_t quota[kHotMaxTriggers], len[kHotMaxTriggers];
            for (uint32_t q = 0; q < nq; ++q) {
                const uint32_t nt = toff[q + 1] - toff[q];
                const uint64_t n = hot_request_plan(mode, 6, off.data(), trig.data() + toff[q], val.data() + toff[q], nt, k, quota, len);
                CHECK(st.words[q] == toff[q] - 5 && st.words[st.n_at + q] == n);
                const bool scratch = hot_is_sorted(mode, n, k) && n > kHotLdsRecords;
                CHECK(st.words[st.slab_at + q] == (scratch ? (uint32_t)slab : kHotNone));
                if (scratch) slab += hot_next_pow2((uint32_t)n);
                for (uint32_t j = 0; j < nt; ++j) {
                    CHECK(st.words[st.trig_at + st.words[q] + j] == trig[toff[q] + j]);
                    if (mode == PG_HOT_TOPIC) CHECK(st.words[st.quota_at + st.words[q] + j] == quota[j]);
                }
            }
            CHECK(st.words[nq] == total && st.slab_records == slab);
        }
    // a request past the limit: refused by name
    const uint32_t trig[5] = {1, 4, 5, 1, 0}, toff[3] = {0, 1, 4};
    HotStage st;
    CHECK(!hot_stage_build("t", PG_HOT_GROUP, 6, off.data(), trig, nullptr, toff, 2, 4, &st, &r) && r.code == PG_ERR_UNSUPPORTED &&
          has(r, "request 1 concatenates 65537 entries"));
    // no triggers at all, no arrays
    const uint32_t none[3] = {9, 9, 9};
    CHECK(hot_stage_build("t", PG_HOT_TOPIC, 6, off.data(), nullptr, nullptr, none, 2, 4, &st, &r) && st.words.size() == 7 && st.slab_records == 0);
}

int main() {
    check_stage();
    check_validate();
    check_args();
    check_quotas();
    check_pieces();
    check_statement();
    if (g_fail) {
        printf("hot: %d checks FAILED\n", g_fail);
        return 1;
    }
    printf("hot OK\n");
    return 0;
}
