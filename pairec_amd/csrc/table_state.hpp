// table_state.hpp — what a table carries beside its rows (pg_table, common.hpp), in two structs with different lifetimes:
//   TableDerived: what is BUILT FROM the rows — shadows, statistics, row norms, the threshold model's moments.  Valid for one
//                 generation of the rows; rebuilt lazily by the ensure_* functions (recall_table.hip, recall_i4.hip, recall_r2.hip).
//   TableLearned: what the plans LEARN about the table from verified batches — hints that tune the next plan, never state an
//                 answer depends on (every plan is verified).  Its update rules are its members, each written once.
// Both travel with the rows in pg_table_swap.  Plain C++17, no HIP: a host compiler builds this header alone (tests/table_state_check.cpp).
// Locking: a table is shared by the contexts of a device (a coalescer's sibling), each under its own ctx->mu, so g_table_state_mu
// guards every write of either struct and every read of `learned`, which the plans read as a SNAPSHOT (a copy taken under the
// mutex).  `derived` is read without it by whoever holds the table's shared lock after the ensure_* call that built what it
// reads.  Lock order: ctx->mu, then the table's rw, then g_table_state_mu (innermost: nothing else is taken under it).
#pragma once
#include <cstdint>
#include <mutex>
#include <type_traits>

namespace pg {

extern std::mutex g_table_state_mu;   // (recall_table.hip)

struct TableDerived {
    // lazily computed for the screened recall (invalidated by upload / fill): statistics and the shadow of
    // the rows that the screen streams instead of the fp32 rows (the exact re-scoring still gathers fp32):
    //   dim 128: int8, X = rint(x / s8) with ONE scale s8 = max|x| / 127 for the table, [rows + 64][dim] bytes
    //            — a quarter of the fp32 bytes; resid8 = max over rows of ||x - s8 X||_2 (measured, not assumed)
    //   dim 64, and dim-128 tables whose value range defeats one int8 scale (heavy tails, outliers): bf16 (RNE of
    //            every fp32 value), [rows + 64][dim] — half the bytes — plus the largest row norm of every 32-row block
    bool stats_valid = false;
    bool all_finite = false;
    float max_norm = 0.0f;       // upper bound of the rows' L2 norms
    uint16_t* d16 = nullptr;     // bf16 shadow; allocated on first use, kept across rebuilds
    float* dnorm2 = nullptr;     // with the bf16 shadow: largest row norm^2 of every 32-row block (the bf16 bound is relative)
    int8_t* d8 = nullptr;        // int8 shadow; likewise
    bool shadow_is_i8 = false;   // which of the two the current statistics belong to
    float s8 = 0.0f;             // int8 scale
    float resid8 = 0.0f;         // upper bound of the rows' quantisation residual (L2)
    bool shadow_failed = false;  // allocation failed once: stay on the exact scan
    float* d_nx = nullptr;       // squared-Euclidean recall: |x|^2 of every row [rows + 64] (lazily, invalidated by upload / fill)
    float* d_nxmin = nullptr;    // ... and the smallest of every 32-row block (the int8 screen's per-block cutoff under that metric)
    bool nx_valid = false;
    float l2_slack = 0.0f;       // mean (|x|^2 - the block's smallest) / 2 in units of the score spread: above Knobs::l2_max_slack the exact scan serves that metric
    // recall_i4.hip: the 4-bit shadow that the full pass of a small batch streams (dim 128, built on the first such
    // recall, 68 B per row): nibbles [rows + 64][64 B], one fp32 scale per row, and the bound's measured constants
    uint8_t* d4 = nullptr;
    uint32_t* d4s = nullptr;     // row scale (bf16, low half) | row residual bound (bf16, high half)
    bool i4_ok = false, i4_failed = false;
    float rho4 = 0.0f;           // max over rows of ||x - x^|| / (s_row sqrt(dim)) (diagnostic)
    float rmax4 = 0.0f;          // max over rows of ||x - x^|| (upper bound)
    float lam4 = 0.0f;           // mean residual term in units of the score spread (decides whether the shadow pays)
    // recall_r2.hip: the int8 RESIDUAL shadow (x = s8 X8 + s8r Xr + e2) that the refinement stage of crowded tables gathers beside
    // the int8 shadow; built the first time the table shows more than Knobs::r2_min_factor screen suspects per answer
    int8_t* d8r = nullptr;
    float s8r = 0.0f, resid2 = 0.0f;   // its scale (s8 / 254), the measured upper bound of ||e2||
    bool r2_ok = false, r2_failed = false;
    // Threshold predictor (recall_plan.hip, built by recall_table.hip; DESIGN.md 4.1, plan 0): a Gaussian model of a query's scores over the rows — mean
    // vector and covariance from a row sample, built with the statistics — and the quantile z = (K-th best score −
    // mean) / sigma actually observed for the batches served so far (TableLearned::pred_*).  Once the observed z is tight, a
    // batch's first thresholds come from the model instead of a pilot sample.  A hint only: every plan is verified, results are exact.
    float* d_pred = nullptr;      // [dim] mean | [dim][dim] covariance | 4 doubles: n, sum z, sum z^2, min z
    bool pred_model = false;      // mean / covariance belong to the current rows

    // the device allocations this struct owns (pg_table_destroy): free_fn(void*) for each one that exists
    template <class F> void for_each_owned(F&& free_fn) const {
        void* const owned[] = {d16, dnorm2, d8, d_nx, d_nxmin, d4, d4s, d8r, d_pred};
        for (void* p : owned) if (p) free_fn(p);
    }
    // rows written (upload / fill): statistics, int8 / bf16 shadow and row norms are rebuilt by the next recall that wants them
    void rows_written() { stats_valid = nx_valid = false; }
    // ensure_table_stats rebuilds: the 4-bit shadow, the residual shadow and the threshold model follow the rows too
    void stats_rebuilt() { i4_ok = i4_failed = r2_ok = r2_failed = pred_model = false; }
};

struct TableLearned {
    float i4m_pairs = 0.0f;      // recall_i4m.hip: running average of the (row, query) pairs its 4-bit stage lets through, per query
    float wide_susp = 0.0f;      // running average of the int8 screen's suspects per query (passes without a 4-bit stage)
    uint32_t rec_scale = 0;      // recall_plan.hip: the 256-query pass's hit-record areas, x their default size (0 = 1; doubled when a batch overflows them)
    uint32_t prefix_failures = 0; // batches whose refined thresholds failed verification for most queries (ordered rows): two → no refinement
    uint32_t pred_k = 0;          // the K the threshold model's observations belong to
    double pred_n = 0.0, pred_sum = 0.0, pred_sum2 = 0.0, pred_min = 0.0, pred_total = 0.0;   // host copy as of the last verified batch
    uint32_t pred_backoff = 0;    // batches that stay on the pilot plan after a prediction failed verification
    uint32_t pred_failures = 0;   // (never reset: the back-off of a table that keeps failing stays long)
    // screened plans that ended in an overflowing suspect / record / candidate list (rows crowded within the screen's error of
    // every query's K-th score: DESIGN.md 4.1): after two in a row the table's recalls start on the exact scan for a while
    uint32_t screen_overflow_streak = 0, screen_backoff = 0;

    // the running averages: seeded by the first sample (0 = unseeded)
    static void average_in(float& avg, float x) { avg = avg > 0.0f ? 0.75f * avg + 0.25f * x : x; }
    void note_wide_susp(float per_q) { average_in(wide_susp, per_q); }
    void note_i4m_pairs(float per_q) { average_in(i4m_pairs, per_q); }

    uint32_t rec_scale_eff() const { return rec_scale ? rec_scale : 1; }
    // a batch overflowed the hit-record areas: they double, up to `max` times their default size; false: they stay
    bool grow_rec_scale(uint32_t max) {
        if (rec_scale_eff() >= max) return false;
        rec_scale = rec_scale ? rec_scale * 2 : 2;
        return true;
    }

    // A prediction failed verification (forget: the observations no longer describe the queries), or held with too many
    // candidates per answer (!forget): the pilot plan serves for an exponentially growing number of batches.
    void pred_failed(bool forget) {
        pred_failures++;
        pred_backoff = 64u << (pred_failures < 6 ? pred_failures : 6);
        if (forget) pred_n = pred_sum = pred_sum2 = 0.0;
    }
    // the device's sums {n, sum z, sum z^2, min z, total} as a verified batch saw them (two streams report: keep the later snapshot)
    void pred_report(const double st[5]) {
        if (st[4] < pred_total) return;
        pred_n = st[0]; pred_sum = st[1]; pred_sum2 = st[2]; pred_min = st[3]; pred_total = st[4];
    }
    // the observations belong to one K (batches already in flight still report the old K's quantiles: four batches stay on the pilot plan)
    void pred_change_k(uint32_t k) { pred_k = k; pred_n = pred_sum = pred_sum2 = 0.0; pred_backoff = 4; }

    void screen_overflowed() { if (++screen_overflow_streak >= 2) screen_backoff = 64; }
    void screen_held() { screen_overflow_streak = 0; }
    // true: this recall starts on the exact scan (and one batch of the back-off is spent)
    bool screen_backed_off() { if (!screen_backoff) return false; screen_backoff--; return true; }

    // The three reset moments.  Separate on purpose: a job verified after a write still reports into this struct, and the rebuilds happen
    // lazily, at the next recall that wants the statistics or the model.
    void rows_written() { screen_overflow_streak = screen_backoff = 0; }
    void stats_rebuilt() { i4m_pairs = wide_susp = 0.0f; rec_scale = prefix_failures = 0; }
    void model_rebuilt() { pred_k = pred_backoff = 0; pred_n = pred_sum = pred_sum2 = pred_total = 0.0; pred_min = 1e300; }
};
static_assert(std::is_trivially_copyable<TableLearned>::value, "a snapshot of TableLearned is a plain copy");

}  // namespace pg
