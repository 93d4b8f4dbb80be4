// traffic_host_san.cpp — a stand-alone program (its own main) that runs TrafficControlSort's host side under ASan + UBSan:
// pg_traffic_compile / pg_traffic_free, pg_traffic_table and pg_traffic_sort_host on hostile values (NaN and +-Inf scores and
// alphas, a `total` of exactly 0, scalars that drive goint out of range) and on a few hundred seeded random configs, refused ones
// among them.  tests/test_traffic_san_cpu.py compiles it together with csrc/traffic.hip — the host code under test, instrumented —
// and links the rest from the built library.  It checks what holds for every answer (the count, every entry of the list once,
// control ids and positions only where an entry is, ascending positions with NaN last, untouched guard words); the answers
// themselves are held against tests/traffic_ref.py by the Python tests.  UBSan is what looks at goint: no cast may see a value
// outside int64.  No GPU is touched: nothing here takes a context.
#include "../include/pairec_gpu.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

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
static const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

struct Call {
    std::vector<pg_traffic_target> targets;
    uint32_t ctx_size = 10, page_no = 1, nq = 1, cap = 1;
    double gamma = 1.0, beta = 1.0, eta = 1.6;
    std::vector<double> score, alpha;
    std::vector<uint8_t> member;
    std::vector<uint32_t> order, count;
    bool with_order = false, with_count = false, with_optional = true;
};

// what holds for every answer
static void check_answer(const Call& c, const uint32_t* out, const uint32_t* out_count, const int32_t* cid, const double* pos, const char* what) {
    for (uint32_t q = 0; q < c.nq; ++q) {
        const size_t q0 = (size_t)q * c.cap;
        const uint32_t n = c.with_count ? std::min(c.count[q], c.cap) : c.cap;
        CHECK(out_count[q] == n, "%s: count %u, expected %u", what, out_count[q], n);
        std::vector<uint8_t> in_list(c.cap, 0), seen(c.cap, 0);
        for (uint32_t j = 0; j < n; ++j) in_list[c.with_order ? c.order[q0 + j] : j] = 1;
        double last = -kInf;
        bool nan_seen = false;
        for (uint32_t k = 0; k < c.cap; ++k) {
            const uint32_t e = out[q0 + k];
            if (k >= n) { CHECK(e == kEmpty, "%s: slot %u behind the count holds %u", what, k, e); continue; }
            CHECK(e < c.cap && in_list[e] && !seen[e], "%s: slot %u holds %u (empty, foreign or twice)", what, k, e);
            if (e >= c.cap) continue;
            seen[e] = 1;
            if (!pos) continue;
            const double p = pos[q0 + e];
            if (p != p) nan_seen = true;
            else {
                CHECK(!nan_seen && p >= last, "%s: slot %u: position %g behind %g (or behind a NaN)", what, k, p, last);
                last = p;
            }
        }
        for (uint32_t e = 0; e < c.cap; ++e) {
            if (cid && !in_list[e]) CHECK(cid[q0 + e] == 0, "%s: element %u is no entry but has control id %d", what, e, cid[q0 + e]);
            if (pos && !in_list[e]) {
                uint64_t b;
                memcpy(&b, &pos[q0 + e], 8);
                CHECK(b == 0x7FF8000000000000ull, "%s: element %u is no entry but has a position", what, e);
            }
            if (cid && in_list[e] && c.targets.empty()) CHECK(cid[q0 + e] >= 1 && (uint32_t)cid[q0 + e] <= c.cap, "%s: identity id %d", what, cid[q0 + e]);
        }
    }
}

static int run(const Call& c, const char* what, bool expect_ok = true) {
    pg_traffic* m = nullptr;
    int rc = pg_traffic_compile(c.targets.data(), (uint32_t)c.targets.size(), &m);
    if (rc != PG_OK) {
        CHECK(!m && (rc == PG_ERR_INVALID || rc == PG_ERR_UNSUPPORTED) && pg_last_error()[0], "%s: compile refused with %d", what, rc);
        return rc;
    }
    CHECK(pg_traffic_num_targets(m) == (int)c.targets.size(), "%s: %d targets", what, pg_traffic_num_targets(m));
    const size_t e = (size_t)c.nq * c.cap;
    std::vector<uint32_t> out(e + 1, kGuard), out_count(c.nq + 1, kGuard);
    std::vector<int32_t> cid(e + 1, (int32_t)kGuard);
    std::vector<double> pos(e + 1, -12345.0);
    const bool T = !c.targets.empty();
    rc = pg_traffic_sort_host(m, c.ctx_size, c.page_no, c.gamma, c.beta, c.eta, c.nq, c.cap, T ? c.score.data() : nullptr, T ? c.member.data() : nullptr,
                              c.with_order ? c.order.data() : nullptr, c.with_count ? c.count.data() : nullptr, T ? c.alpha.data() : nullptr, out.data(),
                              out_count.data(), c.with_optional ? cid.data() : nullptr, c.with_optional ? pos.data() : nullptr);
    CHECK(out[e] == kGuard && out_count[c.nq] == kGuard && cid[e] == (int32_t)kGuard && pos[e] == -12345.0, "%s: a write behind an output", what);
    if (rc == PG_OK) check_answer(c, out.data(), out_count.data(), c.with_optional ? cid.data() : nullptr, c.with_optional ? pos.data() : nullptr, what);
    else CHECK((rc == PG_ERR_INVALID || rc == PG_ERR_UNSUPPORTED) && pg_last_error()[0], "%s: refused with %d", what, rc);
    CHECK(!expect_ok || rc == PG_OK, "%s: %s", what, pg_last_error());
    pg_traffic_free(m);
    return rc;
}

static void tables() {
    static const uint32_t len[4] = {500, 1000, 3000, 10000};
    for (int w = 0; w < 4; ++w) {
        std::vector<double> t(len[w] + 1, -1.0);
        CHECK(pg_traffic_table(w, 0, len[w], t.data()) == PG_OK && t[len[w]] == -1.0, "table %d", w);
        for (uint32_t i = 0; i < len[w]; ++i) CHECK(t[i] == t[i] && t[i] >= 0.0 && t[i] < 3.0, "table %d entry %u = %g", w, i, t[i]);
        CHECK(pg_traffic_table(w, len[w], 1, t.data()) == PG_ERR_INVALID && pg_traffic_table(w, 1, len[w], t.data()) == PG_ERR_INVALID, "table %d: reads past its end", w);
        CHECK(pg_traffic_table(w, len[w], 0, nullptr) == PG_OK, "table %d: an empty read at its end", w);
    }
    double x;
    CHECK(pg_traffic_table(4, 0, 1, &x) == PG_ERR_INVALID && pg_traffic_table(-1, 0, 1, &x) == PG_ERR_INVALID, "an unknown table");
    CHECK(pg_traffic_table(0, 0xFFFFFFFFu, 2, &x) == PG_ERR_INVALID, "a range that wraps");
}

static void hostile() {
    double pos1;
    pg_traffic_table(0, 1, 1, &pos1);
    const double specials[] = {kNaN, kInf, -kInf, 0.0, -0.0, -1.0, 1e308, -1e308, 5e-324, 1e-300, 9.3e18, -9.3e18, 1e19};
    const size_t ns = sizeof specials / sizeof *specials;
    size_t runs = 0;
    for (size_t a = 0; a < ns; ++a)
        for (size_t b = 0; b < ns; ++b)
            for (uint32_t page = 1; page <= 2; ++page) {
                Call c;
                c.targets = {{7, PG_TRAFFIC_PERCENT}, {-9, PG_TRAFFIC_QUANTITY}, {2147483647, PG_TRAFFIC_PERCENT}};
                c.nq = 2;
                c.cap = 9;
                c.ctx_size = page == 1 ? 2 : 0xFFFFFFFFu;
                c.page_no = page;
                c.gamma = specials[(a + b) % ns];
                c.beta = specials[(a + 2 * b + 1) % ns];
                c.eta = specials[(2 * a + b + 2) % ns];
                for (uint32_t i = 0; i < c.nq * c.cap; ++i) {
                    c.score.push_back(i % 4 == 1 ? specials[(a + i) % ns] : 1.0 - 0.01 * i);
                    c.member.push_back((uint8_t)(i * 5 + 3));
                }
                c.score[0] = specials[a];                                   // maxScore
                c.score[c.cap] = pos1;                                      // request 1: total = 0 behind two entries
                c.score[c.cap + 1] = -1.0;
                c.alpha = {specials[b], -2.0, specials[(b + 5) % ns], 1.5, specials[b], -0.0};
                c.with_count = true;
                c.count = {9, 2};
                run(c, "hostile");
                ++runs;
            }
    CHECK(runs == 2 * ns * ns, "%zu hostile runs", runs);
}

static void random_cases() {
    std::mt19937_64 rng(20260202);
    auto below = [&](uint32_t k) { return (uint32_t)(rng() % k); };
    auto unit = [&] { return (double)(rng() >> 11) / 9007199254740992.0; };
    size_t served = 0, refused = 0;
    for (int iter = 0; iter < 400; ++iter) {
        Call c;
        const uint32_t T = below(12) == 0 ? 9 + below(3) : below(9);        // (above 8: refused)
        for (uint32_t t = 0; t < T; ++t)
            c.targets.push_back({below(40) == 0 ? INT32_MIN : (int32_t)below(2000) - 100, below(30) == 0 ? 3 : 1 + (int32_t)below(2)});      // (rarely refused)
        c.nq = below(25) == 0 ? 0 : 1 + below(4);
        c.cap = 1 + below(600);
        c.ctx_size = below(25) == 0 ? 0 : 1 + below(80);
        c.page_no = below(25) == 0 ? 0 : 1 + below(3);
        const double gammas[] = {1.0, 0.0, -1.0, 2.5}, etas[] = {1.6, 0.01, 0.2};
        c.gamma = gammas[below(4)];
        c.beta = 0.1 + 3.0 * unit();
        c.eta = etas[below(3)];
        const size_t e = (size_t)c.nq * c.cap;
        c.score.resize(e);
        c.member.resize(e);
        c.order.resize(e);
        c.count.resize(c.nq);
        c.alpha.resize((size_t)c.nq * T);
        for (size_t i = 0; i < e; ++i) {
            c.score[i] = below(20) ? unit() * (below(5) ? 1.0 : -3.0) : 0.0;
            c.member[i] = (uint8_t)rng();
        }
        const double alphas[] = {0.0, 0.0, 1.0, -1.0, 3.5, -8.0, 0.3, 40.0, -0.02, kNaN, kInf, -kInf};
        for (auto& a : c.alpha) a = alphas[below(below(6) ? 9 : 12)] * (0.5 + unit());
        for (uint32_t q = 0; q < c.nq; ++q) {
            for (uint32_t j = 0; j < c.cap; ++j) c.order[(size_t)q * c.cap + j] = j;
            std::shuffle(c.order.begin() + (size_t)q * c.cap, c.order.begin() + (size_t)(q + 1) * c.cap, rng);
            c.count[q] = below(3) ? c.cap : below(c.cap + 2);
        }
        c.with_order = below(2) != 0;
        c.with_count = below(2) != 0;
        c.with_optional = below(3) != 0;
        if (c.with_order && e && below(30) == 0) c.order[below((uint32_t)e)] = c.cap + below(3);      // (inside a count: refused)
        const int rc = run(c, "random case", false);
        if (rc == PG_OK) ++served; else ++refused;
    }
    CHECK(served >= 200 && refused >= 20, "%zu served, %zu refused", served, refused);
    pg_traffic_free(nullptr);
}

int main() {
    tables();
    hostile();
    random_cases();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("traffic_host_san OK\n");
    return 0;
}
