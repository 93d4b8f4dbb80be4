// Stand-alone check of pairec_amd/csrc/index_serve.hpp (built and run by test_index_serve_cpu.py; host only).  The expected
// values are written out by hand from the rules as the index's host code stated them before they moved into the header.
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "index_serve.hpp"

using namespace pg;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

static void bands() {
    const uint32_t nq[9] = {1, 2, 8, 9, 32, 33, 64, 65, 256};
    const int band[9] = {0, 1, 1, 2, 2, 3, 3, 4, 4};
    for (int i = 0; i < 9; ++i) CHECK(band_of(nq[i]) == band[i]);
    CHECK(kBands == 5);
}

static void countdown() {
    IndexServe sv;
    sv.skip[2].store(3);                                  // the band of 9-32 queries
    CHECK(!serve_take_skip(sv, 8) && !serve_take_skip(sv, 33) && !serve_take_skip(sv, 1) && !serve_take_skip(sv, 256));
    CHECK(sv.skip[2].load() == 3 && sv.skipped_switch.load() == 0);
    CHECK(serve_take_skip(sv, 9) && serve_take_skip(sv, 32) && serve_take_skip(sv, 20));
    CHECK(!serve_take_skip(sv, 20) && !serve_take_skip(sv, 20));      // the fourth batch tries the plan again, and so do later ones
    CHECK(sv.skip[2].load() == 0 && sv.skipped_switch.load() == 3);
    for (int b = 0; b < kBands; ++b) CHECK(sv.skip[b].load() == 0);

    // four threads, 400 batches each, against a switch armed with 1,000
    IndexServe many;
    many.skip[4].store(1000);
    uint32_t took[4] = {0, 0, 0, 0};
    std::vector<std::thread> th;
    for (int i = 0; i < 4; ++i)
        th.emplace_back([&many, &took, i] {
            for (int n = 0; n < 400; ++n) took[i] += serve_take_skip(many, 100) ? 1u : 0u;
        });
    for (auto& t : th) t.join();
    CHECK(took[0] + took[1] + took[2] + took[3] == 1000);
    CHECK(many.skipped_switch.load() == 1000 && many.skip[4].load() == 0);
}

static void verdicts() {
    const uint32_t NF = 1, DENSE = 2, ROUNDS = 4;         // the device's flag bits
    CHECK(kPlanNonfinite == NF && kPlanDense == DENSE && kPlanRounds == ROUNDS);
    // precedence: non-finite, then dense (also with rounds), then rounds, then overflow, then held
    CHECK(plan_verdict(NF | DENSE | ROUNDS, 1) == PlanVerdict::nonfinite);
    CHECK(plan_verdict(NF | DENSE, 0) == PlanVerdict::nonfinite && plan_verdict(NF | ROUNDS, 0) == PlanVerdict::nonfinite);
    CHECK(plan_verdict(DENSE | ROUNDS, 0) == PlanVerdict::dense && plan_verdict(DENSE, 1) == PlanVerdict::dense);
    CHECK(plan_verdict(ROUNDS, 1) == PlanVerdict::rounds);
    CHECK(plan_verdict(0, 1) == PlanVerdict::overflow && plan_verdict(0, 7) == PlanVerdict::overflow);
    CHECK(plan_verdict(0, 0) == PlanVerdict::held);
    CHECK(plan_switch_batches(64) == 64 && plan_switch_batches(0) == 0 && plan_switch_batches(0xFFFFFFFFu) == 0x7FFFFFFF &&
          plan_switch_batches(0x7FFFFFFFu) == 0x7FFFFFFF && plan_switch_batches(0x80000000u) == 0x7FFFFFFF);

    {   // non-finite wins over dense and rounds: its counter alone, nothing armed
        IndexServe sv;
        CHECK(serve_plan_done(sv, 8, NF | DENSE | ROUNDS, 0, 64, 10, 20, 30) == PlanVerdict::nonfinite);
        CHECK(sv.plans.load() == 1 && sv.queries.load() == 8 && sv.replan_nonfinite.load() == 1);
        CHECK(sv.replan_dense.load() == 0 && sv.replan_rounds.load() == 0 && sv.replan_overflow.load() == 0 && sv.plans_held.load() == 0);
        for (int b = 0; b < kBands; ++b) CHECK(sv.skip[b].load() == 0);
        CHECK(sv.pairs.load() == 0 && sv.rows_live.load() == 0 && sv.max_scan.load() == 0);
    }
    {   // dense and rounds together count as dense; dense arms the batch's band with index_skip_batches
        IndexServe sv;
        CHECK(serve_plan_done(sv, 8, DENSE | ROUNDS, 0, 64, 10, 20, 30) == PlanVerdict::dense);
        CHECK(sv.replan_dense.load() == 1 && sv.replan_rounds.load() == 0 && sv.plans_held.load() == 0);
        CHECK(sv.skip[1].load() == 64 && sv.skip[0].load() == 0 && sv.skip[2].load() == 0 && sv.skip[3].load() == 0 && sv.skip[4].load() == 0);
        CHECK(sv.pairs.load() == 0);
    }
    {   // rounds arms too; 0 arms nothing, 0xFFFFFFFF arms 0x7FFFFFFF
        IndexServe sv;
        CHECK(serve_plan_done(sv, 200, ROUNDS, 0, 7, 1, 1, 1) == PlanVerdict::rounds);
        CHECK(sv.replan_rounds.load() == 1 && sv.replan_dense.load() == 0 && sv.skip[4].load() == 7);
        CHECK(serve_plan_done(sv, 1, ROUNDS, 0, 0, 1, 1, 1) == PlanVerdict::rounds);
        CHECK(sv.skip[0].load() == 0 && !serve_take_skip(sv, 1));
        CHECK(serve_plan_done(sv, 40, DENSE, 0, 0xFFFFFFFFu, 1, 1, 1) == PlanVerdict::dense);
        CHECK(sv.skip[3].load() == 0x7FFFFFFF);
        CHECK(sv.plans.load() == 3 && sv.queries.load() == 241);
    }
    {   // overflow alone re-plans without arming
        IndexServe sv;
        CHECK(serve_plan_done(sv, 32, 0, 1, 64, 10, 20, 30) == PlanVerdict::overflow);
        CHECK(sv.replan_overflow.load() == 1 && sv.plans_held.load() == 0 && sv.pairs.load() == 0);
        for (int b = 0; b < kBands; ++b) CHECK(sv.skip[b].load() == 0);
    }
    {   // none of these: held; max_scan is a running maximum
        IndexServe sv;
        CHECK(serve_plan_done(sv, 32, 0, 0, 64, 1000, 500, 70) == PlanVerdict::held);
        CHECK(serve_plan_done(sv, 4, 0, 0, 64, 11, 7, 50) == PlanVerdict::held);
        CHECK(serve_plan_done(sv, 1, 0, 0, 64, 1, 1, 90) == PlanVerdict::held);
        CHECK(sv.plans.load() == 3 && sv.plans_held.load() == 3 && sv.queries.load() == 37 && sv.queries_held.load() == 37);
        CHECK(sv.pairs.load() == 1012 && sv.rows_live.load() == 508 && sv.max_scan.load() == 90);
        CHECK(sv.replan_dense.load() + sv.replan_rounds.load() + sv.replan_overflow.load() + sv.replan_nonfinite.load() == 0);
        for (int b = 0; b < kBands; ++b) CHECK(sv.skip[b].load() == 0);
    }
}

static void fold() {
    IndexServe sv;
    sv.plans = 10; sv.plans_held = 4; sv.queries_held = 40; sv.queries = 100; sv.pairs = 5000; sv.rows_live = 300; sv.max_scan = 77;
    sv.replan_dense = 1; sv.replan_rounds = 2; sv.replan_overflow = 3; sv.replan_nonfinite = 4; sv.skipped_stale = 5; sv.skipped_switch = 6;
    pg_index_stats_t st{};
    st.n_lists = 9; st.dim = 128; st.rows = 1234; st.generation = 3; st.max_radius = 2.5f; st.mean_radius = 1.5f;
    st.largest_list = 17; st.empty_lists = 2; st.build_ms = 12.5;
    st.calls = 1; st.queries = 2; st.rows_scored = 3; st.pairs_scored = 4;
    st.fallback_dense = 5; st.fallback_stale = 6; st.fallback_nonfinite = 7; st.fallback_overflow = 8; st.rows_live = 9; st.max_query_scan_rows = 100;
    serve_fold_stats(sv, &st);
    CHECK(st.calls == 11 && st.queries == 102 && st.rows_scored == 5003 && st.pairs_scored == 5004);
    CHECK(st.fallback_dense == 6 && st.fallback_stale == 6 && st.fallback_nonfinite == 11 && st.fallback_overflow == 11);      // (rounds: no field)
    CHECK(st.rows_live == 309 && st.max_query_scan_rows == 100);
    CHECK(st.n_lists == 9 && st.dim == 128 && st.rows == 1234 && st.generation == 3 && st.max_radius == 2.5f && st.mean_radius == 1.5f &&
          st.largest_list == 17 && st.empty_lists == 2 && st.build_ms == 12.5);
    sv.max_scan = 101;
    pg_index_stats_t st2{};
    st2.max_query_scan_rows = 100;
    serve_fold_stats(sv, &st2);
    CHECK(st2.max_query_scan_rows == 101);
}

static void pre_search() {
    // stale beats non-finite, which beats the L2 dim
    CHECK(index_pre_search(5, 4, true, true, 192) == IndexPre::stale);
    CHECK(index_pre_search(4, 4, true, true, 192) == IndexPre::nonfinite);
    CHECK(index_pre_search(4, 4, false, true, 192) == IndexPre::l2_dim && index_pre_search(4, 4, false, true, 256) == IndexPre::l2_dim);
    CHECK(index_pre_search(4, 4, false, true, 64) == IndexPre::search && index_pre_search(4, 4, false, true, 128) == IndexPre::search);
    CHECK(index_pre_search(4, 4, false, false, 192) == IndexPre::search && index_pre_search(4, 4, false, false, 256) == IndexPre::search);
    CHECK(index_pre_search(3, 4, false, false, 64) == IndexPre::stale);
    CHECK(index_pre_fallback(IndexPre::search) == nullptr);
    CHECK(index_pre_fallback(IndexPre::stale) == &pg_index_stats_t::fallback_stale);
    CHECK(index_pre_fallback(IndexPre::nonfinite) == &pg_index_stats_t::fallback_nonfinite);
    CHECK(index_pre_fallback(IndexPre::l2_dim) == &pg_index_stats_t::fallback_dense);
}

static void refresh() {
    const uint64_t rows = 1000;
    const double frac = 0.25;                             // the full fraction: 250 rows
    CHECK(refresh_plan(2, false, 10, rows, frac, false) == RefreshPlan::refused);
    CHECK(refresh_plan(2, true, 10, rows, frac, false) == RefreshPlan::incremental);
    CHECK(refresh_plan(2, true, 999, rows, frac, false) == RefreshPlan::incremental);       // (mode 2 asks no fraction)
    CHECK(refresh_plan(1, true, 10, rows, frac, false) == RefreshPlan::full);
    CHECK(refresh_plan(0, true, 0, rows, frac, true) == RefreshPlan::full);                 // equal generations under force
    CHECK(refresh_plan(1, true, 0, rows, frac, true) == RefreshPlan::full);
    CHECK(refresh_plan(0, true, 250, rows, frac, false) == RefreshPlan::incremental);       // exactly the fraction
    CHECK(refresh_plan(0, true, 251, rows, frac, false) == RefreshPlan::full);              // one row above
    CHECK(refresh_plan(0, false, 10, rows, frac, false) == RefreshPlan::full);              // uncovered
}

static void build_shape() {
    struct Case { uint64_t rows; uint32_t n_lists_in, lists; uint64_t sample; };
    const Case c[3] = {{63, 0, 1, 63}, {100, 0, 1, 64}, {100000000ull, 0, 40000, 2560000}};
    for (const Case& k : c) {
        const IndexBuildShape s = index_build_shape(k.rows, pg_index_params{k.n_lists_in, 0, 0, 0});
        CHECK(s.n_lists == k.lists && s.train_rows == k.sample && s.iters == 8);
    }
    CHECK(index_build_shape(4194304, pg_index_params{70000, 0, 0, 0}).n_lists == 65536);
    CHECK(kMaxLists == 65536);
    // train_rows below the list count is raised to it, above the row count lowered to it
    const IndexBuildShape lo = index_build_shape(6400, pg_index_params{100, 10, 3, 0});
    CHECK(lo.n_lists == 100 && lo.train_rows == 100 && lo.iters == 3);
    const IndexBuildShape hi = index_build_shape(6400, pg_index_params{100, 7000, 0, 0});
    CHECK(hi.n_lists == 100 && hi.train_rows == 6400 && hi.iters == 8);
    const IndexBuildShape mid = index_build_shape(6400, pg_index_params{100, 500, 1, 0});
    CHECK(mid.train_rows == 500 && mid.iters == 1);
}

struct Entry {                                            // what the cache's policy needs of an entry
    WhereKey key{};
    size_t bytes = 0;
};
static int g_builds = 0;
static auto builder(size_t bytes) {
    return [bytes](std::shared_ptr<Entry>* out) {
        *out = std::make_shared<Entry>();
        (*out)->bytes = bytes;
        ++g_builds;
        return 0;
    };
}

static void cache() {
    const pg_features* fs = reinterpret_cast<const pg_features*>(uintptr_t(0x1000));
    const pg_where* w = reinterpret_cast<const pg_where*>(uintptr_t(0x2000));
    auto key = [&](long long value) { return WhereKey{fs, 2, 7, 4, value, 11, nullptr, 0}; };
    {   // three entries, a hit moves to the front
        WhereCache<Entry> c;
        pg_index_where_stats_t st{};
        std::shared_ptr<Entry> e;
        CHECK(where_cache_get(c, st, 4, key(1), &e, builder(100)) == 0);
        CHECK(where_cache_get(c, st, 4, key(2), &e, builder(200)) == 0);
        CHECK(where_cache_get(c, st, 4, key(3), &e, builder(300)) == 0);
        CHECK(st.builds == 3 && st.hits == 0 && st.entries == 3 && st.bytes == 600 && st.evictions == 0);
        CHECK(c.front()->key == key(3) && c.back()->key == key(1));
        const int before = g_builds;
        CHECK(where_cache_get(c, st, 4, key(1), &e, builder(999)) == 0);
        CHECK(g_builds == before && st.hits == 1 && st.builds == 3 && st.entries == 3 && st.bytes == 600);
        CHECK(e->bytes == 100 && c.front() == e && c.back()->key == key(2));
        // a context with capacity 1 arrives: two go from the back, the bytes fall by their sizes (200 and 300); its key is the front's
        CHECK(where_cache_get(c, st, 1, key(1), &e, builder(999)) == 0);
        CHECK(st.evictions == 2 && st.entries == 1 && st.bytes == 100 && st.hits == 2 && c.size() == 1 && c.front()->key == key(1));
        // ... and a miss at capacity 1 replaces the one entry
        CHECK(where_cache_get(c, st, 1, key(5), &e, builder(50)) == 0);
        CHECK(st.builds == 4 && st.evictions == 3 && st.entries == 1 && st.bytes == 50 && c.front()->key == key(5));
        where_cache_clear(c, st);
        CHECK(c.empty() && st.entries == 0 && st.bytes == 0 && st.builds == 4 && st.evictions == 3);
    }
    {   // capacity 0: every call builds, nothing is kept
        WhereCache<Entry> c;
        pg_index_where_stats_t st{};
        std::shared_ptr<Entry> e;
        for (int i = 0; i < 3; ++i) {
            CHECK(where_cache_get(c, st, 0, key(1), &e, builder(100)) == 0);
            CHECK(e && e->bytes == 100 && e->key == key(1));
        }
        CHECK(st.builds == 3 && st.hits == 0 && st.entries == 0 && st.bytes == 0 && st.evictions == 0 && c.empty());
    }
    {   // a build that fails: its status comes back, nothing is counted or kept
        WhereCache<Entry> c;
        pg_index_where_stats_t st{};
        std::shared_ptr<Entry> e;
        CHECK(where_cache_get(c, st, 4, key(1), &e, [](std::shared_ptr<Entry>*) { return -3; }) == -3);
        CHECK(st.builds == 0 && st.entries == 0 && st.bytes == 0 && c.empty());
    }
    {   // keys that differ in one field only do not match
        const WhereKey k{fs, 2, 7, 4, 5, 11, nullptr, 0};
        CHECK(k == (WhereKey{fs, 2, 7, 4, 5, 11, nullptr, 0}));
        CHECK(!(k == WhereKey{fs, 2, 7, 4, 5, 12, nullptr, 0}));          // generation
        CHECK(!(k == WhereKey{fs, 2, 8, 4, 5, 11, nullptr, 0}));          // column version
        CHECK(!(k == WhereKey{fs, 3, 7, 4, 5, 11, nullptr, 0}) && !(k == WhereKey{fs, 2, 7, 5, 5, 11, nullptr, 0}) &&
              !(k == WhereKey{fs, 2, 7, 4, 6, 11, nullptr, 0}) && !(k == WhereKey{nullptr, 2, 7, 4, 5, 11, nullptr, 0}));
        const WhereKey cw{fs, -1, 0, 0, 0, 11, w, 21};
        CHECK(cw == (WhereKey{fs, -1, 0, 0, 0, 11, w, 21}));
        CHECK(!(cw == WhereKey{fs, -1, 0, 0, 0, 11, w, 22}));             // epoch
        CHECK(!(cw == WhereKey{fs, -1, 0, 0, 0, 11, nullptr, 21}));
        WhereCache<Entry> c;
        pg_index_where_stats_t st{};
        std::shared_ptr<Entry> e;
        CHECK(where_cache_get(c, st, 4, k, &e, builder(1)) == 0);
        CHECK(where_cache_get(c, st, 4, WhereKey{fs, 2, 7, 4, 5, 12, nullptr, 0}, &e, builder(1)) == 0);
        CHECK(where_cache_get(c, st, 4, WhereKey{fs, 2, 8, 4, 5, 11, nullptr, 0}, &e, builder(1)) == 0);
        CHECK(where_cache_get(c, st, 4, cw, &e, builder(1)) == 0);
        CHECK(where_cache_get(c, st, 4, WhereKey{fs, -1, 0, 0, 0, 11, w, 22}, &e, builder(1)) == 0);
        CHECK(st.builds == 5 && st.hits == 0 && st.evictions == 1 && st.entries == 4);
    }
}

int main() {
    bands();
    countdown();
    verdicts();
    fold();
    pre_search();
    refresh();
    build_shape();
    cache();
    if (g_failed) {
        std::printf("index_serve: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("index_serve OK\n");
    return 0;
}
