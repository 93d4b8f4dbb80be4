// Stand-alone check of pairec_amd/csrc/table_state.hpp (built and run by test_table_state_cpu.py; host only).  The expected
// values are written out from the rules as the recall code stated them before they moved into the header.
#include <array>
#include <cstdint>
#include <cstdio>
#include <utility>

#include "table_state.hpp"

using pg::TableDerived;
using pg::TableLearned;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

// Every field of the two structs, through structured bindings: a field added to a struct and not here does not compile.
constexpr int kLearnedFields = 14, kDerivedFields = 28;
enum { I4M_PAIRS, WIDE_SUSP, REC_SCALE, PREFIX_FAILURES, PRED_K, PRED_N, PRED_SUM, PRED_SUM2, PRED_MIN, PRED_TOTAL, PRED_BACKOFF,
       PRED_FAILURES, STREAK, SCREEN_BACKOFF };
using LearnedValues = std::array<double, kLearnedFields>;
using DerivedValues = std::array<double, kDerivedFields>;

static LearnedValues values(const TableLearned& l) {
    const auto& [a, b, c, d, e, f, g, h, i, j, k, m, n, o] = l;
    return {(double)a, (double)b, (double)c, (double)d, (double)e, f, g, h, i, j, (double)k, (double)m, (double)n, (double)o};
}
// field i = base + i: distinct, non-zero, exact in every field's type
static TableLearned filled_learned(int base) {
    TableLearned l;
    auto& [a, b, c, d, e, f, g, h, i, j, k, m, n, o] = l;
    int v = base;
    a = (float)v++; b = (float)v++; c = v++; d = v++; e = v++; f = v++; g = v++; h = v++; i = v++; j = v++; k = v++; m = v++; n = v++; o = v++;
    return l;
}
static LearnedValues filled_values(int base) {
    LearnedValues r;
    for (int i = 0; i < kLearnedFields; ++i) r[i] = base + i;
    return r;
}

struct Put {                     // flags take `flag`, numbers and pointers a value of their own
    int v;
    bool flag;
    void operator()(bool& x) { x = flag; ++v; }
    void operator()(float& x) { x = (float)v++; }
    template <class T> void operator()(T*& p) { p = reinterpret_cast<T*>((uintptr_t)64 * v++); }
};
struct Get {
    double operator()(bool x) const { return x ? 1.0 : 0.0; }
    double operator()(float x) const { return x; }
    template <class T> double operator()(T* p) const { return (double)reinterpret_cast<uintptr_t>(p); }
};
static TableDerived filled_derived(int base, bool flag) {
    TableDerived t;
    auto& [a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, p, q, r, s, u, v, w, x, y, z, aa, ab, ac] = t;
    Put put{base, flag};
    put(a); put(b); put(c); put(d); put(e); put(f); put(g); put(h); put(i); put(j); put(k); put(l); put(m); put(n);
    put(o); put(p); put(q); put(r); put(s); put(u); put(v); put(w); put(x); put(y); put(z); put(aa); put(ab); put(ac);
    return t;
}
static DerivedValues values(const TableDerived& t) {
    const auto& [a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, p, q, r, s, u, v, w, x, y, z, aa, ab, ac] = t;
    const Get get;
    return {get(a), get(b), get(c), get(d), get(e), get(f), get(g), get(h), get(i), get(j), get(k), get(l), get(m), get(n),
            get(o), get(p), get(q), get(r), get(s), get(u), get(v), get(w), get(x), get(y), get(z), get(aa), get(ab), get(ac)};
}

static void check_running_average() {
    TableLearned l;
    CHECK(l.wide_susp == 0.0f && l.i4m_pairs == 0.0f);             // zero: unseeded
    l.note_wide_susp(100.0f);
    CHECK(l.wide_susp == 100.0f);                                  // the first sample seeds it
    l.note_wide_susp(200.0f);
    CHECK(l.wide_susp == 125.0f);                                  // 0.75 x 100 + 0.25 x 200
    l.note_wide_susp(200.0f);
    CHECK(l.wide_susp == 143.75f);                                 // 0.75 x 125 + 0.25 x 200
    CHECK(l.i4m_pairs == 0.0f);
    l.note_i4m_pairs(100.0f);
    CHECK(l.i4m_pairs == 100.0f);
    l.note_i4m_pairs(200.0f);
    CHECK(l.i4m_pairs == 125.0f);
    l.note_i4m_pairs(200.0f);
    CHECK(l.i4m_pairs == 143.75f);
    CHECK(l.wide_susp == 143.75f);
}

static void check_rec_scale() {
    TableLearned l;
    CHECK(l.rec_scale == 0 && l.rec_scale_eff() == 1);
    const uint32_t walk[] = {2, 4, 8, 16};
    for (uint32_t want : walk) {
        CHECK(l.grow_rec_scale(16));
        CHECK(l.rec_scale == want && l.rec_scale_eff() == want);
    }
    CHECK(!l.grow_rec_scale(16));
    CHECK(l.rec_scale == 16);
    TableLearned never;
    CHECK(!never.grow_rec_scale(1));                               // max = 1: never
    CHECK(never.rec_scale == 0 && never.rec_scale_eff() == 1);
}

static void check_predictor() {
    const uint32_t want[] = {128, 256, 512, 1024, 2048, 4096, 4096, 4096};     // 64 << min(failures, 6)
    TableLearned l;
    for (int i = 0; i < 8; ++i) {
        l.pred_n = 5.0; l.pred_sum = 6.0; l.pred_sum2 = 7.0; l.pred_min = 8.0; l.pred_total = 9.0;
        const bool forget = i % 2 == 0;
        l.pred_failed(forget);
        CHECK(l.pred_failures == (uint32_t)i + 1 && l.pred_backoff == want[i]);
        if (forget) CHECK(l.pred_n == 0.0 && l.pred_sum == 0.0 && l.pred_sum2 == 0.0);     // a failed prediction starts over
        else CHECK(l.pred_n == 5.0 && l.pred_sum == 6.0 && l.pred_sum2 == 7.0);            // too many candidates: it keeps them
        CHECK(l.pred_min == 8.0 && l.pred_total == 9.0);
    }
    // either kind alone walks the same back-off
    for (int kind = 0; kind < 2; ++kind) {
        TableLearned m;
        for (int i = 0; i < 8; ++i) {
            m.pred_failed(kind == 0);
            CHECK(m.pred_backoff == want[i]);
        }
    }
    // snapshots: the later one wins, an equal total is accepted, a smaller one ignored
    TableLearned s;
    const double first[5] = {10.0, 20.0, 30.0, 0.5, 100.0}, older[5] = {1.0, 2.0, 3.0, 0.25, 99.0}, same[5] = {11.0, 21.0, 31.0, 0.4, 100.0};
    s.pred_report(first);
    CHECK(s.pred_n == 10.0 && s.pred_sum == 20.0 && s.pred_sum2 == 30.0 && s.pred_min == 0.5 && s.pred_total == 100.0);
    s.pred_report(older);
    CHECK(s.pred_n == 10.0 && s.pred_sum == 20.0 && s.pred_sum2 == 30.0 && s.pred_min == 0.5 && s.pred_total == 100.0);
    s.pred_report(same);
    CHECK(s.pred_n == 11.0 && s.pred_sum == 21.0 && s.pred_sum2 == 31.0 && s.pred_min == 0.4 && s.pred_total == 100.0);
    // change of K: the observations start over, four batches stay on the pilot plan; nothing else moves
    TableLearned k = filled_learned(1);
    LearnedValues want_k = filled_values(1);
    k.pred_change_k(500);
    want_k[PRED_K] = 500;
    want_k[PRED_N] = want_k[PRED_SUM] = want_k[PRED_SUM2] = 0;
    want_k[PRED_BACKOFF] = 4;
    CHECK(values(k) == want_k);
}

static void check_screen_overflow() {
    TableLearned l;
    l.screen_overflowed();
    CHECK(l.screen_overflow_streak == 1 && l.screen_backoff == 0);           // one overflow: no back-off
    l.screen_held();
    CHECK(l.screen_overflow_streak == 0);
    l.screen_overflowed();
    CHECK(l.screen_backoff == 0);                                            // a held plan in between: the streak starts over
    l.screen_overflowed();
    CHECK(l.screen_overflow_streak == 2 && l.screen_backoff == 64);          // two in a row
    for (int i = 0; i < 64; ++i) {
        CHECK(l.screen_backed_off());
        CHECK(l.screen_backoff == (uint32_t)(63 - i));
    }
    CHECK(!l.screen_backed_off());                                           // the 65th recall screens again
    CHECK(l.screen_backoff == 0);
    CHECK(l.screen_overflow_streak == 2);                                    // (the countdown does not touch the streak)
}

static void check_reset_moments() {
    TableLearned w = filled_learned(1), s = filled_learned(1), m = filled_learned(1);
    LearnedValues want = filled_values(1);
    w.rows_written();
    want[STREAK] = want[SCREEN_BACKOFF] = 0;
    CHECK(values(w) == want);

    want = filled_values(1);
    s.stats_rebuilt();
    want[I4M_PAIRS] = want[REC_SCALE] = want[WIDE_SUSP] = want[PREFIX_FAILURES] = 0;
    CHECK(values(s) == want);

    want = filled_values(1);
    m.model_rebuilt();
    want[PRED_K] = want[PRED_N] = want[PRED_SUM] = want[PRED_SUM2] = want[PRED_TOTAL] = want[PRED_BACKOFF] = 0;
    want[PRED_MIN] = 1e300;
    CHECK(values(m) == want);                                                // (pred_failures is reset nowhere)

    // the derived side of a write and of a statistics rebuild: flags only, every pointer and constant stays
    TableDerived d = filled_derived(1, true);
    d.rows_written();
    CHECK(!d.stats_valid && !d.nx_valid);
    d.stats_valid = d.nx_valid = true;
    CHECK(values(d) == values(filled_derived(1, true)));
    d.stats_rebuilt();
    CHECK(!d.i4_ok && !d.i4_failed && !d.r2_ok && !d.r2_failed && !d.pred_model);
    d.i4_ok = d.i4_failed = d.r2_ok = d.r2_failed = d.pred_model = true;
    CHECK(values(d) == values(filled_derived(1, true)));
}

static void check_swap_and_owned() {
    TableLearned la = filled_learned(1), lb = filled_learned(101);
    std::swap(la, lb);
    CHECK(values(la) == filled_values(101) && values(lb) == filled_values(1));
    for (int i = 0; i < kLearnedFields; ++i) CHECK(values(la)[i] != values(lb)[i]);

    TableDerived da = filled_derived(1, true), db = filled_derived(101, false);
    const DerivedValues va = values(da), vb = values(db);
    for (int i = 0; i < kDerivedFields; ++i) CHECK(va[i] != vb[i]);           // distinct in every field
    std::swap(da, db);
    CHECK(values(da) == vb && values(db) == va);

    // the owned allocations: each of the nine pointers once, none when there is none
    int n = 0;
    uintptr_t sum = 0;
    da.for_each_owned([&](void* p) { ++n; sum += reinterpret_cast<uintptr_t>(p); });
    const void* const owned[] = {da.d16, da.dnorm2, da.d8, da.d_nx, da.d_nxmin, da.d4, da.d4s, da.d8r, da.d_pred};
    uintptr_t want = 0;
    for (const void* p : owned) want += reinterpret_cast<uintptr_t>(p);
    CHECK(n == 9 && sum == want);
    n = 0;
    TableDerived().for_each_owned([&](void*) { ++n; });
    CHECK(n == 0);
}

int main() {
    check_running_average();
    check_rec_scale();
    check_predictor();
    check_screen_overflow();
    check_reset_moments();
    check_swap_and_owned();
    if (g_failed) {
        std::printf("table_state: %d check(s) FAILED\n", g_failed);
        return 1;
    }
    std::printf("table_state OK\n");
    return 0;
}
