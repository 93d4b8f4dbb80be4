// recall_plan.hip — the plans of a recall: which launches of the table pass (recall.hip) a batch gets, in which order, and what a
// verified batch teaches the table.  Host code, plus the small kernels that keep a plan's books (initial state, the threshold
// model's per-query moments and observations, the refinement's verification, the status block).
//
// The pass's kernels are reached through the launchers of recall_shared.hpp only: a plan names no template argument and no grid.
// The plans' arithmetic — sample geometry, seed rank, chunk schedule, hit-record areas — is recall_plan_math.hpp, which a host
// compiler checks alone (tests/recall_plan_math_check.cpp).
// Locking: callers hold ctx->mu.  pg_table::learned is read through snapshots taken under g_table_state_mu, a fresh one where
// rec_scale is read (recall_job_check doubles it and the same plan runs again).
#include "common.hpp"
#include "recall_shared.hpp"

namespace pg {

// a job's status block, packed on the device by status_pack_kernel and copied to the host in ONE piece: [0] overflow flag,
// [1 + q] valid count of query q, then
constexpr uint32_t kPredStatsAt = 260;        // words [260, 270): the table's observation sums (five doubles)
constexpr uint32_t kI4mStatAt = 272;          // [272] the (row, query) pairs the 4-bit stage of a mid-batch pass let through,
                                              // [+1] suspects of the full pass's last launch, [+2] a hit-record area overflowed,
                                              // [+3] pairs that reached the exact re-scoring, [+4] candidates the pass collected
constexpr uint32_t kStatusCopyWords = kI4mStatAt + 5;
static_assert(kStatusCopyWords <= 300 && kStatusCopyWords <= kRecallStatusWords, "the status block ends in front of the words other calls keep in ctx->h_status");
// (an index plan has none of the words above: its own twelve take their place, index.hip)
static_assert(kIndexStatAt > kMaxQueries && kIndexStatAt + 12 <= kStatusCopyWords, "an index plan's status words");

// (launched <<<1, kMaxQueries>>>; null pointers = words that stay zero)
__global__ void status_pack_kernel(const uint32_t* __restrict__ overflow, uint32_t nq, uint32_t rec_ovf_word,
                                   const uint32_t* __restrict__ pred_stats, const uint32_t* __restrict__ pairs_word,
                                   const uint32_t* __restrict__ susp, const uint32_t* __restrict__ rescored,
                                   const uint32_t* __restrict__ cand_seen, uint32_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    uint32_t v1 = (susp && t < nq) ? susp[t] : 0u, v3 = (rescored && t < nq) ? rescored[t] : 0u, v4 = (cand_seen && t < nq) ? cand_seen[t] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v1 += __shfl_xor(v1, off, 64);
        v3 += __shfl_xor(v3, off, 64);
        v4 += __shfl_xor(v4, off, 64);
    }
    __shared__ uint32_t s[3][4];
    if ((t & 63) == 0) { s[0][t >> 6] = v1; s[1][t >> 6] = v3; s[2][t >> 6] = v4; }
    out[1 + t] = t < nq ? overflow[1 + t] : 0u;
    if (t < 10) out[kPredStatsAt + t] = pred_stats ? pred_stats[t] : 0u;
    __syncthreads();
    if (t == 0) {
        out[0] = overflow[0];
        out[kI4mStatAt] = pairs_word ? *pairs_word : 0u;
        out[kI4mStatAt + 1] = s[0][0] + s[0][1] + s[0][2] + s[0][3];
        out[kI4mStatAt + 2] = overflow[rec_ovf_word];
        out[kI4mStatAt + 3] = s[1][0] + s[1][1] + s[1][2] + s[1][3];
        out[kI4mStatAt + 4] = s[2][0] + s[2][1] + s[2][2] + s[2][3];
    }
}

// after a refined pilot plan: thr = score of the K-th best candidate kept (select_kernel), thr_ref = the raised threshold
__global__ void refine_verify_kernel(const float* __restrict__ thr, const float* __restrict__ thr_ref,
                                     uint32_t* __restrict__ count, uint32_t nq) {
    const uint32_t q = threadIdx.x;
    if (q < nq && !(thr[q] >= thr_ref[q])) count[q] = 0u;
}

__global__ void recall_init_kernel(const float* __restrict__ queries, uint32_t nq, uint32_t dim,
                                   float* __restrict__ qpad, float* __restrict__ thr,
                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ overflow) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kMaxQueries * dim) qpad[i] = (i / dim) < nq ? queries[i] : 0.0f;
    if (i < kMaxQueries) {
        thr[i] = -__builtin_inff();
        cnt[i] = 0;
        cnt[kMaxQueries + i] = 0;                          // susp_cnt (RecallScratch: right behind cnt)
    }
    if (i == 0) { *overflow = 0; overflow[kRecOvfWord] = 0; }
}

// (the threshold predictor's model and what it is for: recall_table.hip, at pred_moments_kernel)
// per query: mean mu.q and sigma sqrt(q'Sq) of its scores (one workgroup of 128 threads per query)
__global__ __launch_bounds__(128) void pred_query_kernel(const float* __restrict__ qpad, const float* __restrict__ pred,
                                                         float* __restrict__ ms, float* __restrict__ thr, float z_lo) {
    __shared__ float qs[128];
    __shared__ double red[2][2];
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    qs[t] = qpad[(size_t)q * 128 + t];
    __syncthreads();
    const float* S = pred + 128;
    float sq = 0.0f;
    for (int i = 0; i < 128; ++i) sq = __fmaf_rn(S[i * 128 + t], qs[i], sq);          // (S q)_t: S symmetric, column t coalesced
    double v = (double)sq * (double)qs[t], m = (double)pred[t] * (double)qs[t];
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_xor(v, off, 64);
        m += __shfl_xor(m, off, 64);
    }
    if ((t & 63) == 0) { red[t >> 6][0] = v; red[t >> 6][1] = m; }
    __syncthreads();
    if (t == 0) {
        const double var = red[0][0] + red[1][0], mean = red[0][1] + red[1][1];
        const float m = (float)mean, sg = var > 0.0 ? (float)sqrt(var) : 0.0f;
        ms[2 * q] = m;
        ms[2 * q + 1] = sg;
        if (thr) {
            // first threshold from the model: mean + z_lo sigma, rounded down; anything odd → +inf, which leaves the query
            // without candidates: the plan check then sends the batch to the pilot plan.  (Query columns >= nq keep the
            // -inf recall_init_kernel gave them.)
            float t = __fmaf_rn(z_lo, sg, m);
            t = t - fabsf(t) * 1e-6f;
            if (!(sg > 0.0f) || !(t == t) || fabsf(t) > 1e30f) t = __builtin_inff();
            thr[q] = t;
        }
    }
}
// after a verified-to-be pass: fold the batch's observed quantiles into the table's statistics (queries that came up
// short of K, or whose model sigma is 0, do not count), then they travel to the host with the status words
__global__ void pred_update_kernel(const float* __restrict__ thr, const float* __restrict__ ms, const uint32_t* __restrict__ cnt,
                                   uint32_t nq, uint32_t k, double* __restrict__ stats) {
    const uint32_t q = threadIdx.x;
    double z = 0.0, z2 = 0.0, n = 0.0, mn = 1e300;
    if (q < nq && cnt[q] >= k && ms[2 * q + 1] > 0.0f) {
        const float t = thr[q];
        if (t == t && fabsf(t) < 1e30f) {
            z = ((double)t - (double)ms[2 * q]) / (double)ms[2 * q + 1];
            z2 = z * z;
            n = 1.0;
            mn = z;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        z += __shfl_xor(z, off, 64);
        z2 += __shfl_xor(z2, off, 64);
        n += __shfl_xor(n, off, 64);
        const double o = __shfl_xor(mn, off, 64);
        mn = o < mn ? o : mn;
    }
    if ((q & 63) == 0 && n > 0.0) {
        atomicAdd(&stats[4], n);                       // observations ever (orders the host's snapshots; never decays)
        atomicAdd(&stats[0], n);
        atomicAdd(&stats[1], z);
        atomicAdd(&stats[2], z2);
        // (min via compare-and-swap on the bit pattern: the values are positive in every workload this is for, and a
        //  stale minimum only makes the margin more careful)
        unsigned long long* a = reinterpret_cast<unsigned long long*>(&stats[3]);
        unsigned long long old = *a;
        while (__longlong_as_double((long long)old) > mn) {
            const unsigned long long seen = atomicCAS(a, old, (unsigned long long)__double_as_longlong(mn));
            if (seen == old) break;
            old = seen;
        }
    }
    // a sliding window in effect: past 2^17 observations the sums halve, so a drifting query population moves the
    // model within ~100 batches (the halving may race another stream's add and drop it: these are statistics)
    __syncthreads();
    if (q == 0 && stats[0] >= 131072.0) {
        stats[0] *= 0.5;
        stats[1] *= 0.5;
        stats[2] *= 0.5;
    }
}

int recall_scratch(pg_ctx* ctx, uint32_t dim, uint32_t k, RecallScratch* rs) {
    const uint32_t cap = k + kCandSlack;
    int rc;
    // the small regions stay packed as they always were (alignment = the element's own), but for the 64-byte fragment loads
    if ((rc = scratch_carve(ctx, kSlotRecallSmall, [&](Carve& c) {
            rs->qpad = c.take<float>((size_t)kMaxQueries * dim);
            rs->qb16 = c.take<uint4>((size_t)kScreenMaxNQB * (dim / 16) * 64, 16);
            rs->thr = c.take<float>(kMaxQueries, 4);
            rs->eps = c.take<float>(kMaxQueries, 4);
            rs->thr_screen = c.take<float>(kMaxQueries, 4);
            rs->cnt = c.take<uint32_t>(kMaxQueries, 4);
            rs->susp_cnt = c.take<uint32_t>(kMaxQueries, 4);
            rs->overflow = c.take<uint32_t>(64 + kMaxQueries, 4);      // ONE region: the overflow word, the valid counts [kMaxQueries] right behind it (+ 1), padding
            rs->qscale = c.take<float>(kMaxQueries, 4);
            rs->q4 = c.take<uint32_t>(160, 4);                         // 4 x 128 B + 4 x 16 B
            rs->thr_ref = c.take<float>(kMaxQueries, 4);
            rs->pred_ms = c.take<float>(2 * (size_t)kMaxQueries, 4);
            rs->susp2_cnt = c.take<uint32_t>(kI4mMaxQueries + 2, 4);   // + two statistics words
            rs->q4m = c.take<uint32_t>(kQ4mWords, 64);                 // (16-byte fragment loads)
            rs->q16 = c.take<uint32_t>((size_t)kMaxQueries * (2 * 32 + 4), 64);   // [256][32] Qh | [256][32] Ql | [256][4]
            rs->susp2w_cnt = c.take<uint32_t>(kMaxQueries + 2, 4);
            rs->status = c.take<uint32_t>(kRecallStatusWords + kMaxQueries, 64);  // ONE region, copied out together: the status words, then cnt_seen
            rs->cnt_seen = rs->status + kRecallStatusWords;
        }))) return rc;
    const size_t lists = (size_t)kMaxQueries * cap;
    if ((rc = scratch_carve(ctx, kSlotRecallCand, [&](Carve& c) {
            rs->cand[0] = c.take<uint64_t>(lists);
            rs->cand[1] = c.take<uint64_t>(lists);
            rs->susp = c.take<uint32_t>(lists);
            rs->susp2 = c.take<uint32_t>(lists);
        }))) return rc;
    rs->cap = cap;
    return PG_OK;
}

// ---------------------------------------------------------------------------------------------
// One recall = one batch of queries against one table (one table pass when the first plan holds).
// Plans, tried in order until one completes without overflowing a candidate list:
//  pilot — the threshold comes from a jittered 1/S block sample (its K'-th best score, K' chosen six
//          sigma above the expected rank K/S, so it is below the true K-th best except with
//          negligible probability), then ONE full-rate pass over the whole table collects every row
//          at or above it.  Verified exactly: if a query ends with fewer than min(K, rows)
//          candidates the sample lied and the next plan runs.  ~1.5 K candidates per query instead
//          of K ln(rows/32768) for the growing-chunk plan.  On big tables the pass is split after its first
//          quarter and the thresholds are raised to the k2-th best candidate found so far (a 16x larger sample:
//          ~1.2 K candidates per query for the rest); the raised threshold is verified against the K-th best
//          score that comes out.  Batches of <= 4 queries stream the 4-bit shadow instead (recall_i4.hip).
//  grow  — geometric chunks, threshold refreshed after each (small tables, and the fallback).
//  safe  — bounded chunks that cannot overflow (adversarially ordered tables).
// A plan is ENQUEUED as a whole (no host synchronisation inside it) and VERIFIED afterwards from a few status
// words copied to pinned host memory: recall_dev_locked synchronises right away, the device-resident pipelines
// (pipeline.hip) defer the check to the end of the whole request batch, so the rank / fusion / sort stages of a
// batch are queued behind its recall without the GPU ever waiting for the host.
// ---------------------------------------------------------------------------------------------
enum RecallPlan { kPilot = 0, kGrow = 1, kSafe = 2, kPredict = 3 };

static inline uint64_t rs_cap_bound(uint32_t k) { return (uint64_t)k + kCandSlack; }

int recall_job_prepare(RecallJob* j) {
    pg_ctx* ctx = j->ctx;
    const pg_table* t = j->t;
    const Knobs& kn = ctx->knobs;
    int rc;
    if (j->l2) {
        if (t->dim != 64 && t->dim != 128) {
            set_error("recall (squared Euclidean): dim=%u unsupported (64 or 128)", t->dim);
            return PG_ERR_UNSUPPORTED;
        }
        if ((rc = ensure_table_nx(ctx, t))) return rc;
    }
    j->table_gen = t->generation.load(std::memory_order_relaxed);
    j->rows_qualified = (uint32_t)t->rows;
    if (j->filter.col && j->filter.admitted >= 0) {
        j->rows_qualified = (uint32_t)j->filter.admitted;
    } else if (j->filter.col) {
        // how many rows the filter admits: the plan check needs it (a filtered list may rightly be shorter than K), and the
        // pilot plan is only worth its launches when the sample holds enough of them
        void* p;
        if ((rc = scratch_reserve(ctx, kSlotStatus, 4096, &p))) return rc;
        unsigned long long* d_n = reinterpret_cast<unsigned long long*>((char*)p + 3072);
        PG_HIP(hipMemsetAsync(d_n, 0, 8, ctx->stream));
        if ((rc = filter_count_launch(ctx, j->filter, t->rows, d_n))) return rc;
        unsigned long long h_n = 0;
        PG_HIP(hipMemcpyAsync(&h_n, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        j->rows_qualified = (uint32_t)h_n;
        j->filter.admitted = (long long)h_n;      // (the re-run of a failed query does not count again)
    }
    if ((rc = recall_scratch(ctx, t->dim, j->k, &j->rs))) return rc;
    j->d_count = j->rs.overflow + 1;              // status words in one block: one device → host copy
    j->rows = (uint32_t)t->rows;
    j->nblocks = (j->rows + kPieceRows - 1) / kPieceRows;
    j->scan_ms = j->total_ms = 0.0;
    j->scanned_rows = 0;
    j->scan_bytes = 0;
    j->scan_launches = 0;
    j->next_plan = 0;
    j->enqueued_plan = -1;
    j->failed.clear();

    // Policy: finite tables of dim <= 128 use the screened scan (int8 or bf16 filter + exact re-scoring) for every
    // batch size (knobs.screen_min = 0), HBM-bound up to 128 queries per pass; everything else rides the exact
    // fp32-MFMA scan in groups of <= 64 queries, one launch per group.
    bool screen = j->nq > kn.screen_min && t->dim <= 128 && !kn.recall_exact && !j->exact_only;
    if (screen) {
        if ((rc = ensure_table_stats(ctx, t))) return rc;
        if (!t->derived.stats_valid || !t->derived.all_finite) screen = false;      // no shadow (dim, memory) or non-finite rows
    }
    TableLearned seen;                                 // what the policy below reads of pg_table::learned: one snapshot
    {
        std::lock_guard<std::mutex> state_guard(g_table_state_mu);
        if (screen && t->learned.screen_backed_off()) screen = false;   // this table's screened plans kept overflowing: exact scan for now
        seen = t->learned;
    }
    // squared Euclidean: the int8 screen with per-block cutoffs for up to 128 queries (dim 128, int8 shadow); else the exact scan
    if (j->l2 && !(screen && t->dim == 128 && t->derived.shadow_is_i8 && j->nq <= 128 && !kn.l2_exact)) screen = false;
    // rows of (nearly) one norm: one cutoff per 32-row block; beyond: the per-row test (three VALU instructions per bound instead of half a one)
    j->l2_per_row = j->l2 && screen && t->derived.l2_slack > kn.l2_max_slack;
    j->screen = screen;
    j->screen4 = j->screen4m = false;
    j->n_plans = 0;
    const uint32_t rows = j->rows;
    const SampleGeometry sg = sample_geometry(rows, j->k, j->rows_qualified, kn.pilot_fraction, kn.pilot_sigmas);
    j->stride = sg.stride;
    j->sample_blocks = 0;
    j->k_pilot = 0;
    j->perm_mul = 1;
    if (sg.stride >= 2 && !kn.no_pilot) {
        j->sample_blocks = sg.sample_blocks;
        j->k_pilot = sg.k_pilot;
        j->perm_mul = sg.perm_mul;
        if (sg.pilot) j->plans[j->n_plans++] = kPilot;
    }
    j->plans[j->n_plans++] = kGrow;
    j->plans[j->n_plans++] = kSafe;
    if (j->skip_pilot && j->plans[0] == kPilot) j->next_plan = 1;    // the re-run of a query a sampled threshold failed
    static_assert(kIndexPlan != kPilot && kIndexPlan != kGrow && kIndexPlan != kSafe && kIndexPlan != kPredict, "plan ids");
    // small batches: the pilot plan's full pass is HBM-bound on the shadow it streams — use the 4-bit one (recall_i4.hip)
    if (screen && t->dim == 128 && j->nq <= kI4MaxQueries && j->plans[0] == kPilot && !kn.no_screen_i4 &&
        rows >= kn.i4_min_rows && (uint64_t)kMaxQueries * rs_cap_bound(j->k) / kI4MaxQueries < 0xFFFFFFFFull) {
        if ((rc = ensure_table_i4(ctx, t))) return rc;
        // (measured at 100M x 128, int8 pass 2.1 ms: uniform rows, lambda 0.8: 1.37 / 1.38 / 1.59 / 1.66 ms at 1..4
        // queries; Gaussian rows, lambda 1.3: 1.46 / 1.59 / 1.78 / 2.02 — every query re-scores its own suspects)
        static const double kLamScale[kI4MaxQueries] = {1.0, 1.0, 0.88, 0.7};
        j->screen4 = t->derived.i4_ok && (double)t->derived.lam4 <= kn.i4_max_lambda * kLamScale[j->nq - 1];
    }
    // 1 .. 64 queries, inner product, int8 main shadow: the same 4-bit shadow through the matrix pipe, suspects thinned on the int8
    // shadow (recall_i4m.hip) — also for one or two queries (1.08 against the vector screen's 1.17 ms per 100 M rows: its int8 stage
    // re-scores a twentieth of the suspects)
    if (screen && !j->l2 && t->dim == 128 && t->derived.shadow_is_i8 && j->nq >= kn.i4m_min_queries && j->nq <= kI4mMaxQueries &&
        j->nq <= kn.i4m_max_queries && j->plans[0] == kPilot && !kn.no_screen_i4m && rows >= kn.i4_min_rows) {
        if ((rc = ensure_table_i4(ctx, t))) return rc;
        // every pair the 4-bit stage lets through is one random 128-B read (~35 G/s in rescreen8_kernel): beyond i4m_max_pairs of them per pass
        // the int8 shadow's wider stream is the shorter pass.  The count per query is the table's own running average.
        // (two query blocks: the 4-bit stage is vector-ALU-bound, 1.5 instead of 1.2 ms per 100 M rows — the budget shrinks with the gain)
        j->screen4m = t->derived.i4_ok && (double)t->derived.lam4 <= kn.i4m_max_lambda &&
                      (double)seen.i4m_pairs * j->nq <= kn.i4m_max_pairs * (j->nq > 32 ? 0.7 : 1.0);
        if (j->screen4m) j->screen4 = false;
    }
    // crowded rows (clustered embeddings: many suspects per answer): the int8 screen's suspects pass a two-digit refinement on the
    // residual shadow before the exact re-scoring (recall_r2.hip); passes with a 4-bit stage have their own int8 stage
    j->stage2 = false;
    if (screen && !j->l2 && t->dim == 128 && t->derived.shadow_is_i8 && !j->screen4m && !j->screen4 && !kn.no_r2 &&
        (double)seen.wide_susp > kn.r2_min_factor * (double)j->k) {
        if ((rc = ensure_table_r2(ctx, t))) return rc;
        j->stage2 = t->derived.r2_ok;
    }
    // the threshold model: observe with every pilot-plan batch of a big int8-screened table; predict once the observed
    // quantile is tight (plan 0)
    j->predict = j->pred_observe = false;
    // (batches of <= 4 queries too: their full pass — the 4-bit shadow's — takes the same float thresholds, and the pilot's five
    //  launches are 0.15 ms of a lone request's 1.45)
    if (screen && !j->l2 && !j->filter.col && t->dim == 128 && t->derived.shadow_is_i8 && j->plans[0] == kPilot && !j->skip_pilot && !kn.no_predict &&
        rows >= kn.predict_min_rows && j->k < rows / 64) {
        if ((rc = ensure_pred_model(ctx, t))) return rc;
        std::lock_guard<std::mutex> state_guard(g_table_state_mu);
        TableLearned& ln = t->learned;
        if (t->derived.pred_model) {
            if (ln.pred_k != j->k) {                   // the observations belong to one K
                PG_HIP(hipMemsetAsync(t->derived.d_pred + 128 + 128 * 128, 0, 24, ctx->stream));
                ln.pred_change_k(j->k);
            }
            // (a mature model learns nothing from a lone request: its two launches and the 40-byte copy are spared)
            j->pred_observe = !(j->nq <= (uint32_t)kI4MaxQueries && ln.pred_n >= 8192.0);
            if (ln.pred_backoff > 0) {
                --ln.pred_backoff;
            } else if (ln.pred_n >= 1024.0) {
                const double mean = ln.pred_sum / ln.pred_n;
                const double var = ln.pred_sum2 / ln.pred_n - mean * mean;
                const double sd = var > 0.0 ? sqrt(var) : 0.0;
                // tight enough to beat the sample's own six-sigma margin (a threshold 3 % low in z doubles the rows that reach it)
                if (mean > 0.5 && sd <= 0.025 * mean) {
                    j->predict = true;
                    j->z_lo = mean - kn.predict_sigmas * sd - 0.002 * mean;
                    for (int i = j->n_plans; i > 0; --i) j->plans[i] = j->plans[i - 1];
                    j->plans[0] = kPredict;
                    j->n_plans++;
                }
            }
        }
    }
    // a table with an attached index: its plan goes in front of everything above (index.hip; the plans above stay as they are
    // and serve the batch when it does not hold)
    return index_plan_prepare(j);
}

namespace {
struct PlanRun {                     // the launches of one plan (helper of recall_job_enqueue)
    RecallJob* j;
    pg_ctx* ctx;
    const pg_table* t;
    RecallScratch& rs;
    uint32_t n_ev = 0;
    int cur = 0;
    bool susp2_clean = false;        // screen4m_prep_kernel left the mid-batch pass's second counters at zero (same)
    bool susp_clean = true;          // recall_init_kernel left the suspect counters at zero: the plan's first screened launch skips its memset
    bool no_i8 = false;              // the plan launches no int8 / bf16 screen (thresholds predicted, full pass on the 4-bit shadow):
                                     // its integer-unit thresholds are not needed
    bool last_full_screened = false; // the plan's last scan launch was a screened one ...
    bool last_was_i4m = false;       // ... of the mid-batch kind (its survivors are counted in susp2_cnt)
    bool last_was_r2 = false;        // ... followed by the refinement stage (its survivors are counted in susp2w_cnt)
    bool exact_chunks = false;       // every chunk on the exact scan: the safe plan of a FILTERED recall.  Its thresholds stay open until K
                                     // admitted rows were seen — under a selective filter, for many chunks — and a screened chunk with open
                                     // thresholds makes every row a suspect of every query: the hit-record regions are sized for the bounded
                                     // chunk spread evenly over the waves, the waves' shares are not even.  The exact scan stages admitted
                                     // rows only, at most the chunk's rows per query.

    explicit PlanRun(RecallJob* job) : j(job), ctx(job->ctx), t(job->t), rs(job->rs) {}

    // records event i of the job's pool on the stream (the pool grows on demand); nothing when the stage timers are off
    int record_event(size_t i) {
        if (!j->timers) return PG_OK;
        std::vector<hipEvent_t>& pool = *j->events;
        while (pool.size() <= i) {
            hipEvent_t e;
            PG_HIP(hipEventCreate(&e));
            pool.push_back(e);
        }
        PG_HIP(hipEventRecord(pool[i], ctx->stream));
        return PG_OK;
    }

    // one scan launch over logical blocks [rb, rb+cb) of a stride-`st` view, bracketed by HIP events:
    // their sum is the per-pass duration of the dominant kernel that bench.py prices against HBM
    int scan_range(uint32_t rb, uint32_t cb, uint32_t st, bool thr_is_open, bool allow_i4 = false) {
        int rc2;
        if ((rc2 = record_event(2 * n_ev))) return rc2;
        last_full_screened = j->screen && !thr_is_open && !exact_chunks;
        if ((rc2 = last_full_screened ? screened_range(rb, cb, st, allow_i4) : exact_range(rb, cb, st))) return rc2;
        j->scanned_rows += (uint64_t)cb * kPieceRows;
        if ((rc2 = record_event(2 * n_ev + 1))) return rc2;
        ++n_ev;
        return PG_OK;
    }

    // the hit-record areas of a > 128-query launch on the int8 shadow (record_areas, recall_plan_math.hpp), their counters zeroed
    int carve_records(ScreenArgs& sa) {
        // (tables whose batches overflowed these areas got larger ones.  A fresh snapshot: recall_job_check doubles it and the same plan runs again)
        const RecordAreas ra = record_areas((uint32_t)ctx->num_cus, j->k, table_learned(t).rec_scale_eff(), sa.early_share);
        const uint32_t rec_waves = (uint32_t)ctx->num_cus * 8u;
        int rc2;
        if ((rc2 = scratch_carve(ctx, kSlotHitRecords, [&](Carve& c) {
                sa.rec_cnt = c.take<uint32_t>((size_t)rec_waves + 1);
                sa.rec = (char*)c.bytes(ra.bytes);      // the wave regions, then the spill pool
            }))) return rc2;
        sa.rec_cap = ra.cap_w;
        sa.rec_pool = sa.rec + (size_t)rec_waves * ra.cap_w * kRecBytes;
        sa.rec_pool_cap = ra.pool_cap;
        sa.rec_waves = rec_waves;
        PG_HIP(hipMemsetAsync(sa.rec_cnt, 0, (size_t)(rec_waves + 1) * 4, ctx->stream));
        return PG_OK;
    }

    // a screened launch — the int8 / bf16 screen, or under allow_i4 one of the 4-bit passes — and the exact re-scoring of its suspects
    int screened_range(uint32_t rb, uint32_t cb, uint32_t st, bool allow_i4) {
        const uint32_t nq = j->nq;
        const bool i8 = t->derived.shadow_is_i8;
        ScreenArgs sa;
        sa.tab16 = i8 ? (const void*)t->derived.d8 : (const void*)t->derived.d16;
        sa.blk_norm2 = t->derived.dnorm2;
        sa.eps_unit = rs.eps;
        sa.qb16 = rs.qb16;
        sa.thr_screen = rs.thr_screen;
        sa.susp_cnt = rs.susp_cnt;
        sa.susp = rs.susp;
        sa.overflow = rs.overflow;
        sa.cap = rs.cap;
        sa.nq = nq;
        sa.rb_begin = rb;
        sa.rb_end = rb + cb;
        sa.row_end = j->rows;
        sa.stride = st;
        sa.perm_mul = j->perm_mul;
        sa.perm_mod = j->sample_blocks;
        // > 128 queries on the int8 shadow: the scan leaves hit records, which screen_launch decodes into the suspect lists
        const bool records = i8 && nq > 128;
        sa.early_share = records ? ctx->knobs.screen_early_share : ctx->knobs.screen_early_share_narrow;
        sa.blk_nxmin = j->l2 && !j->l2_per_row ? t->derived.d_nxmin : nullptr;
        sa.nx_rows = j->l2 && j->l2_per_row ? t->derived.d_nx : nullptr;
        sa.l2_b = j->l2 ? rs.thr_ref : nullptr;    // (no refinement step under this metric: its buffer carries B_q)
        int rc2;
        if (records && (rc2 = carve_records(sa))) return rc2;
        if (!susp_clean) PG_HIP(hipMemsetAsync(rs.susp_cnt, 0, sizeof(uint32_t) * kMaxQueries, ctx->stream));
        susp_clean = false;
        // the full pass of a small batch streams the 4-bit shadow; its few suspect lists share the whole buffer
        // (whole 64-row groups: a range starts on an even block and ends on one or at the table's end)
        const bool whole64 = allow_i4 && st == 1 && (rb & 1) == 0 && (((rb + cb) & 1) == 0 || rb + cb == j->nblocks);
        const bool i4 = j->screen4 && whole64, i4m = j->screen4m && whole64;
        const uint32_t scap = i4 ? rs.cap * (uint32_t)(kMaxQueries / kI4MaxQueries) : rs.cap;
        const uint64_t r_begin = (uint64_t)rb * kPieceRows;
        const uint64_t r_end = (uint64_t)(rb + cb) * kPieceRows < j->rows ? (uint64_t)(rb + cb) * kPieceRows : j->rows;
        last_was_i4m = i4m;
        if (i4) {
            if ((rc2 = screen4_launch(ctx, t, rs, nq, (uint32_t)r_begin, (uint32_t)r_end, scap, j->l2 ? rs.pred_ms : nullptr))) return rc2;
            j->scan_bytes += (r_end - r_begin) * (j->l2 ? 72 : 68);      // (squared Euclidean: + the row's |x|^2)
        } else if (i4m) {
            // stage-1 suspects share the whole buffer ([nq][4 cap]); what passes the int8 stage lands in susp2 ([nq][cap])
            if ((rc2 = screen4m_launch(ctx, t, rs, nq, (uint32_t)r_begin, (uint32_t)r_end, rs.cap * (uint32_t)(kMaxQueries / kI4mMaxQueries), susp2_clean))) return rc2;
            susp2_clean = false;
            j->scan_bytes += (r_end - r_begin) * 68;
        } else {
            if ((rc2 = screen_launch(ctx, t->dim, i8, sa))) return rc2;
            j->scan_bytes += (uint64_t)cb * kPieceRows * t->dim * (i8 ? 1 : 2);
        }
        // crowded rows: the suspects once more with two more digits (recall_r2.hip); what is left goes to the exact re-scoring
        last_was_r2 = j->stage2 && i8 && !i4 && !i4m && !j->l2 && t->dim == 128;
        if (last_was_r2 && (rc2 = rescreen16_launch(ctx, t, rs, nq))) return rc2;
        // exact re-scoring of the launch's suspects → candidate keys: of the lists a second stage thinned (susp2, with that stage's
        // counters), else of the screen's own
        const bool thinned = last_was_r2 || i4m;
        return rescore_launch(ctx, t->dim, j->l2, t->d, rs.qpad, rs.thr, thinned ? rs.susp2 : rs.susp,
                              last_was_r2 ? rs.susp2w_cnt : (i4m ? rs.susp2_cnt : rs.susp_cnt), thinned ? rs.cap : scap, rs.cnt, rs.cand[cur],
                              rs.overflow, rs.cap, nq, j->rows, j->l2 ? t->derived.d_nx : nullptr, j->l2 ? rs.pred_ms : nullptr,
                              i4 ? screen4_rescore_blocks() : 0, j->filter);
    }

    // exact scan (the first chunk of a screened recall too: its threshold is still -inf,
    // every row is a candidate and there is nothing to screen) in groups of <= 64 queries,
    // one launch; blockIdx.y walks the groups
    int exact_range(uint32_t rb, uint32_t cb, uint32_t st) {
        ScanArgs a;
        a.tab = t->d;
        a.qpad = rs.qpad;
        a.thr = rs.thr;
        a.cnt = rs.cnt;
        a.cand = rs.cand[cur];
        a.overflow = rs.overflow;
        a.cap = rs.cap;
        a.nq = j->nq;
        a.group_q = j->nq > (uint32_t)kMaxQueriesExact ? (uint32_t)kMaxQueriesExact : 0u;
        a.nq_launch = a.group_q ? a.group_q : j->nq;
        a.rb_begin = rb;
        a.rb_end = rb + cb;
        a.row_end = j->rows;
        a.stride = st;
        a.perm_mul = j->perm_mul;
        a.perm_mod = j->sample_blocks;
        a.nx = j->l2 ? t->derived.d_nx : nullptr;
        a.nqv = j->l2 ? rs.pred_ms : nullptr;
        a.filter = j->filter;
        j->scan_bytes += (uint64_t)cb * kPieceRows * t->dim * 4;
        return dispatch_scan(ctx, t->dim, a);
    }

    // keep the best `kk` candidates per query, refresh the thresholds, swap the ping-pong lists
    // last: no launch screens against these thresholds any more (the screen's integer cutoffs are not derived)
    int refresh(uint32_t kk, bool last = false) {
        int rc2;
        if ((rc2 = launch_select(ctx, j->nq, rs.cand[cur], rs.cand[cur ^ 1], rs.cnt, rs.thr, rs.cap, kk, 0, rs.cnt_seen))) return rc2;
        if (j->screen && !no_i8 && !(last && !j->l2) && (rc2 = screen_thr_launch(ctx, t, rs, j->l2, j->l2_per_row))) return rc2;
        cur ^= 1;
        return PG_OK;
    }
    // raise the thresholds to every query's kk-th best candidate so far (lists untouched; inner product only)
    int refine(uint32_t kk) {
        int rc2;
        if ((rc2 = launch_select(ctx, j->nq, rs.cand[cur], rs.cand[cur ^ 1], rs.cnt, rs.thr, rs.cap, kk, 1))) return rc2;
        return j->screen ? screen_thr_launch(ctx, t, rs, false, false) : PG_OK;
    }
    // geometric chunks over `nb` logical blocks of a stride-`st` view, keeping the best `kk` (next_chunk_blocks, recall_plan_math.hpp)
    int grow_scan(uint32_t nb, uint32_t st, uint32_t kk, double growth, bool safe) {
        for (uint32_t rb = 0; rb < nb;) {
            const uint32_t cb = next_chunk_blocks(rb, nb, kk, growth, safe);
            int rc2;
            if ((rc2 = scan_range(rb, cb, st, rb == 0))) return rc2;
            rb += cb;
            if ((rc2 = refresh(kk))) return rc2;
        }
        return PG_OK;
    }

    // ---- the phases of recall_job_enqueue, in its order ----
    bool observe = false;            // this plan contributes its observed quantiles to the table's threshold model
    bool refined = false;            // the pilot plan raised its thresholds after the first quarter of the full pass

    // 1. the padded queries and initial state; the queries in every shadow's format the plan streams; the model's moments
    int prepare_queries(int plan) {
        int rc;
        recall_init_kernel<<<(kMaxQueries * t->dim + 255) / 256, 256, 0, ctx->stream>>>(
            j->d_queries, j->nq, t->dim, rs.qpad, rs.thr, rs.cnt, rs.overflow);
        PG_HIP(hipGetLastError());
        // (squared Euclidean: |q|^2 of every padded query; the threshold model is off: its buffer is free)
        if (j->l2 && (rc = query_norm2_launch(ctx, rs.qpad, kMaxQueries, t->dim, rs.pred_ms))) return rc;
        // thresholds predicted and the full pass on the 4-bit shadow: the plan launches no int8 screen, so neither the int8 query
        // fragments nor the integer-unit thresholds are needed (two launches less in front of a lone request, two behind)
        no_i8 = plan == kPredict && j->screen4;
        if (j->screen) {
            if (!no_i8 && (rc = screen_prep_launch(ctx, t, rs, j->nq, j->nq > 128 && !j->l2))) return rc;
            if (j->screen4 && (rc = screen4_prep_launch(ctx, t, rs))) return rc;
            if (j->screen4m) {
                if ((rc = screen4m_prep_launch(ctx, rs, j->nq))) return rc;
                susp2_clean = true;
            }
            if (j->stage2 && (rc = rescreen16_prep_launch(ctx, t, rs, j->nq))) return rc;
        }
        observe = j->pred_observe && (plan == kPilot || plan == kPredict);
        if (observe || plan == kPredict) {
            // mean and sigma of every query's scores; under prediction the same launch writes the first thresholds
            pred_query_kernel<<<j->nq, 128, 0, ctx->stream>>>(rs.qpad, t->derived.d_pred, rs.pred_ms, plan == kPredict ? rs.thr : nullptr,
                                                              (float)j->z_lo);
            PG_HIP(hipGetLastError());
        }
        return PG_OK;
    }

    // (of 2a) the pilot plan's sample: leaves the thresholds at the sample's K'-th best score
    int pilot_sample() {
        const Knobs& kn = ctx->knobs;
        int rc;
        // The sample itself is streamed in two launches when it is screened: a seed of `seed_rows` rows
        // (exact, every row a candidate) whose m0-th best score becomes the threshold of ONE screened
        // launch over the rest of the sample; m0 is chosen so that fewer than K' sample rows reaching
        // that threshold has probability < 1e-9 (seed_rank, recall_plan_math.hpp);
        // should it happen anyway, select_kernel leaves the threshold at -inf, the full pass overflows
        // and the next plan takes over.  (Measured against geometric chunks over the sample: 1.0 → 0.7 ms.)
        const uint32_t seed_rows = kn.seed_rows;
        const uint64_t sample_rows = (uint64_t)j->sample_blocks * kPieceRows;
        if (j->screen && kn.pilot_growth <= 0.0 && sample_rows > 8ull * seed_rows && j->k_pilot < seed_rows / 4) {
            const uint32_t sb = seed_rows / kPieceRows;
            if ((rc = scan_range(0, sb, j->stride, true))) return rc;
            if ((rc = refresh(seed_rank(seed_rows, j->k_pilot, sample_rows)))) return rc;
            if ((rc = scan_range(sb, j->sample_blocks - sb, j->stride, false))) return rc;
            return refresh(j->k_pilot);
        }
        // geometric chunks over the sample (exact scan, or pilot_growth set: A/B runs)
        return grow_scan(j->sample_blocks, j->stride, j->k_pilot, kn.pilot_growth > 0.0 ? kn.pilot_growth : 8.0, false);
    }

    // 2a. the sampled plans: first thresholds from the pilot sample or the model, then ONE full pass, split for the refinement
    int sampled_plan(int plan) {
        const Knobs& kn = ctx->knobs;
        int rc;
        if (plan == kPredict) {
            // no sample: the first thresholds are the model's (pred_query_kernel), here in the int8 screen's units
            if (!no_i8 && (rc = screen_thr_launch(ctx, t, rs, false, false))) return rc;
        } else {
            if ((rc = pilot_sample())) return rc;
            PG_HIP(hipMemsetAsync(rs.cnt, 0, sizeof(uint32_t) * kMaxQueries, ctx->stream));    // (kPredict: still zero from recall_init_kernel)
        }
        // The sample's threshold is deliberately low (K' = m + 6 sqrt(m) + 8 of a 1/64 sample: ~1.8 K rows reach it where K
        // are needed), and every row that reaches it costs a suspect's hit path and an exact re-scoring — a quarter of
        // the 256-query pass.  After the first quarter of the table the candidates found so far ARE a 16x larger sample:
        // their k2-th best (k2 from the same formula) is a much tighter threshold for the other three quarters.  A
        // contiguous prefix is not a random sample: if the prefix holds more than its share of the best rows the raised
        // threshold can exceed the true K-th score — which is CHECKED after the pass (refine_verify_kernel: the K-th
        // best score that came out must reach the raised threshold), and such a query is re-run like one whose sample
        // threshold was too high.  Randomly ordered rows fail with the sample's own probability (six sigma).
        const uint32_t nb_q = refine_split(j->nblocks);
        const uint32_t k2 = refine_rank(j->k, kn.pilot_sigmas);
        // (not behind a predicted threshold: that one already sits tighter than what a quarter of the table can certify —
        //  rank ~1.1 K against k2's ~1.18 K — so the split would only add a launch boundary)
        refined = j->screen && !j->l2 && !j->screen4 && !kn.no_refine && j->rows >= kn.refine_min_rows && nb_q >= 64 &&
                  k2 < j->k && table_learned(t).prefix_failures < 2 && plan != kPredict;
        if (refined) {
            if ((rc = scan_range(0, nb_q, 1, false, true))) return rc;
            if ((rc = refine(k2))) return rc;
            PG_HIP(hipMemcpyAsync(rs.thr_ref, rs.thr, sizeof(float) * kMaxQueries, hipMemcpyDeviceToDevice, ctx->stream));
            if ((rc = scan_range(nb_q, j->nblocks - nb_q, 1, false, true))) return rc;
        } else if ((rc = scan_range(0, j->nblocks, 1, false, true))) {
            return rc;
        }
        // (statistics: the candidates the full pass collected, before the select keeps K of each list — a predicted threshold that
        //  admits many times K is no use to the table, recall_job_check)
        // (select_kernel notes them in rs.cnt_seen)
        return refresh(j->k, true);
    }

    // 2b. the chunked plans: grow, and safe with its bounded chunks
    int chunked_plan(int plan) {
        // measured: growth 4 is best for the exact scan, 2 for the screened scan whose re-scoring
        // gathers 512 B per staged candidate
        exact_chunks = plan == kSafe && j->filter.col;
        const double growth = ctx->knobs.chunk_growth > 1.0 ? ctx->knobs.chunk_growth : (j->screen && !exact_chunks ? 2.0 : 4.0);
        return grow_scan(j->nblocks, 1, j->k, growth, plan == kSafe);
    }

    // 3. the answers in their final order, what verifies and observes the plan, and the status block on its way to the host
    int finish(int plan) {
        int rc;
        if ((rc = final_launch(ctx, rs.cand[cur], rs.cnt, rs.cap, j->nq, j->k, t->row_offset, j->d_out_rows,
                               j->d_out_scores, j->d_count)))
            return rc;
        const uint64_t n = (uint64_t)j->nq * j->k;
        // a filtered view answers with its source's row ids
        if (t->d_row_map && (rc = compact_map_rows_launch(ctx, j->d_out_rows, n, t->d_row_map, t->map_offset, t->rows))) return rc;
        // (squared Euclidean) the lists were ranked by -d: the distances go out
        if (j->l2 && (rc = negate_launch(ctx, j->d_out_scores, n))) return rc;
        if (refined) {
            // Two thresholds were in force during the full pass, so "K candidates were found" no longer proves that none
            // of the true top K was rejected: the raised one must not exceed the K-th best score that came out — then at
            // least K rows reach it, and every row it rejected is below K rows that were kept.  A query that fails reports
            // zero items, which the plan check reads as "re-run this query" (the same path as a sample threshold that
            // turned out too high).
            refine_verify_kernel<<<1, kMaxQueries, 0, ctx->stream>>>(rs.thr, rs.thr_ref, j->d_count, j->nq);
            PG_HIP(hipGetLastError());
        }
        uint32_t* const pred_stats = observe ? reinterpret_cast<uint32_t*>(t->derived.d_pred + 128 + 128 * 128) : nullptr;
        if (observe) {
            // the K-th best scores that came out (rs.thr after the last refresh) as quantiles of the model; queries that
            // failed report 0 items and do not count.  The sums travel to the host with the status words.
            pred_update_kernel<<<1, kMaxQueries, 0, ctx->stream>>>(rs.thr, rs.pred_ms, j->d_count, j->nq, j->k < j->rows ? j->k : j->rows,
                                                                   reinterpret_cast<double*>(pred_stats));
            PG_HIP(hipGetLastError());
        }
        j->susp_stat = j->screen && (plan == kPilot || plan == kPredict) && last_full_screened;
        j->stat_wide = j->susp_stat && !last_was_i4m;
        // the status words in one block, one copy (they were six copies and two sums of their own: ~40 us of a small batch's step):
        // [kI4mStatAt] the pairs a mid-batch pass's 4-bit stage let through (zero otherwise), [+ 1] the suspects its int8 stage / the
        // int8 screen handed on in the full pass's last launch, [+ 3] what reached the exact re-scoring: the same, or the survivors
        // of the refinement stage, [+ 4] the candidates the pass collected (select_kernel notes them before it keeps K)
        const uint32_t* const susp = j->susp_stat ? (last_was_i4m ? rs.susp2_cnt : rs.susp_cnt) : nullptr;
        status_pack_kernel<<<1, kMaxQueries, 0, ctx->stream>>>(
            rs.overflow, j->nq, kRecOvfWord, pred_stats,
            j->susp_stat && last_was_i4m ? rs.susp2_cnt + kI4mMaxQueries : nullptr, susp, j->susp_stat && last_was_r2 ? rs.susp2w_cnt : susp,
            j->susp_stat ? rs.cnt_seen : nullptr, rs.status);
        PG_HIP(hipGetLastError());
        if (j->d_out_count)
            PG_HIP(hipMemcpyAsync(j->d_out_count, j->d_count, 4 * j->nq, hipMemcpyDeviceToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(j->h_status, rs.status, 4 * (size_t)kStatusCopyWords, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    }
};
}  // namespace

int recall_job_enqueue(RecallJob* j) {
    pg_ctx* ctx = j->ctx;
    if (j->next_plan >= j->n_plans) {
        set_error("recall: candidate overflow in safe mode (internal error)");
        return PG_ERR_DEVICE;
    }
    const int plan = j->plans[j->next_plan];
    int rc;
    // another call on this context may have grown the scratch arenas since recall_job_prepare (a re-plan reaches
    // here long after it): fetch the pointers again rather than trust the cached ones
    if ((rc = recall_scratch(ctx, j->t->dim, j->k, &j->rs))) return rc;
    j->d_count = j->rs.overflow + 1;
    if (plan == kIndexPlan) return index_plan_enqueue(j, kStatusCopyWords);
    PlanRun r(j);
    if ((rc = r.prepare_queries(plan))) return rc;
    // events 0/1 of the pool bracket the whole plan; its scan launches use the pairs after them
    r.n_ev = 1;
    j->timers = !ctx->timers_off;
    if ((rc = r.record_event(0))) return rc;
    if ((rc = plan == kPilot || plan == kPredict ? r.sampled_plan(plan) : r.chunked_plan(plan))) return rc;
    if ((rc = r.record_event(1))) return rc;
    if ((rc = r.finish(plan))) return rc;
    j->n_ev = r.n_ev;
    j->refined = r.refined;
    j->enqueued_plan = plan;
    j->observed = r.observe;
    j->next_plan++;
    return PG_OK;
}

int recall_job_check(RecallJob* j, bool* ok_out) {
    pg_ctx* ctx = j->ctx;
    const int plan = j->enqueued_plan;
    float ms = 0.f;
    if (j->timers) PG_HIP(hipEventElapsedTime(&ms, (*j->events)[0], (*j->events)[1]));
    j->total_ms += ms;
    for (uint32_t i = 1; j->timers && i < j->n_ev; ++i) {
        PG_HIP(hipEventElapsedTime(&ms, (*j->events)[2 * i], (*j->events)[2 * i + 1]));
        j->scan_ms += ms;
        if (ctx->knobs.debug_scan) fprintf(stderr, "[pg] plan %d scan launch %u: %.3f ms\n", plan, i - 1, ms);
    }
    if (ctx->knobs.debug_scan && j->screen) {          // suspects of the last screened launch vs K (developer aid)
        uint32_t sc[4] = {0, 0, 0, 0};
        PG_HIP(hipMemcpy(sc, j->rs.susp_cnt, sizeof sc, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pg] plan %d last screened launch: suspects of queries 0-3: %u %u %u %u (K = %u)\n", plan, sc[0], sc[1], sc[2], sc[3], j->k);
        if (j->t->derived.shadow_is_i8 && j->nq > 128 && scratch_peek(ctx, kSlotHitRecords)) {     // hit records: the fullest wave region, the spill pool
            const uint32_t waves = (uint32_t)ctx->num_cus * 8u;
            std::vector<uint32_t> rc(waves + 1);
            PG_HIP(hipMemcpy(rc.data(), scratch_peek(ctx, kSlotHitRecords), rc.size() * 4, hipMemcpyDeviceToHost));
            uint32_t mx = 0;
            uint64_t sum = 0;
            for (uint32_t w = 0; w < waves; ++w) { mx = rc[w] > mx ? rc[w] : mx; sum += rc[w]; }
            fprintf(stderr, "[pg] plan %d last screened launch: hit records %llu in wave regions (fullest %u), %u in the spill pool\n", plan,
                    (unsigned long long)sum, mx, rc[waves]);
        }
    }
    j->scan_launches += j->n_ev - 1;
    if (plan == kIndexPlan) return index_plan_check(j, ok_out);
    bool ok = j->h_status[0] == 0;
    j->failed.clear();
    if (ok && (plan == kPilot || plan == kPredict)) {
        const uint32_t have = j->filter.col ? j->rows_qualified : j->rows;
        const uint32_t want = j->k < have ? j->k : have;
        for (uint32_t q = 0; q < j->nq; ++q)
            if (j->h_status[1 + q] != want) {
                ok = false;
                j->failed.push_back(q);
            }
    }
    // what the verified batch teaches about the table: one locked section, the update rules are TableLearned's members
    std::lock_guard<std::mutex> state_guard(g_table_state_mu);
    TableLearned& ln = j->t->learned;
    if (j->observed || plan == kPredict) {
        if (j->observed && ln.pred_k == j->k) {
            double st[5];
            memcpy(st, j->h_status + kPredStatsAt, sizeof st);
            ln.pred_report(st);
        }
        if (ctx->knobs.debug_scan && ln.pred_n > 0.0) {
            const double mean = ln.pred_sum / ln.pred_n, var = ln.pred_sum2 / ln.pred_n - mean * mean;
            fprintf(stderr, "[pg] plan %d %s: threshold model n = %.0f, z mean %.5f sd %.5f min %.5f (z_lo of this job %.5f)\n", plan,
                    ok ? "held" : "FAILED", ln.pred_n, mean, var > 0 ? sqrt(var) : 0.0, ln.pred_min, j->z_lo);
        }
        if (plan == kPredict && !ok) {
            // the model's threshold was too high for some query: this table stays on the pilot plan for a while (the
            // whole batch re-runs when more than a handful failed — that must stay rare)
            // and the model starts over: what it learnt no longer describes the queries
            ln.pred_failed(true);
            PG_HIP(hipMemsetAsync(j->t->derived.d_pred + 128 + 128 * 128, 0, 24, ctx->stream));
        }
    }
    if (j->screen) {
        // A screened plan that OVERFLOWED (not: a threshold a few queries' lists fell short of) says the rows crowd within the
        // screen's error of the K-th scores — nearly collinear rows and queries along them: 1 % of 40 M rows within the int8
        // margin of every query's threshold — and the chunked fallback plans would screen the same crowd chunk by chunk (256
        // queries, 40 M such rows: 180 ms shuffled, 790 ms in ascending order, where the exact scan takes 30).  The job's
        // remaining plans run on the exact scan; two such batches in a row and the table's next 64 start there.
        if (j->h_status[0] != 0 && j->h_status[kI4mStatAt + 2] != 0 && ln.grow_rec_scale(ctx->knobs.max_rec_scale)) {
            // the hit-record areas of the 256-query pass were too small for this table (clustered rows: a query's whole cluster sits
            // within the screen's error of its K-th score — tens of suspects per answer where uniform rows have two): they grow, and
            // the same plan runs again; the table keeps the larger areas
            ctx->stats.recall_record_growths++;
            if (j->next_plan > 0) j->next_plan--;
            if (ctx->knobs.debug_scan) fprintf(stderr, "[pg] plan %d overflowed its hit-record areas: scale -> %u, again\n", plan, ln.rec_scale);
        } else if (j->h_status[0] != 0) {
            ctx->stats.recall_screen_overflows++;
            j->screen = j->screen4 = j->screen4m = j->l2_per_row = false;
            j->pred_observe = false;
            // (... starting over at the pilot plan: on the exact scan the sample's threshold is as good as anywhere, while the
            //  growing-chunk plans meet a table in ascending order with a flood of candidates per chunk)
            for (int p = 0; p < j->n_plans; ++p)
                if (j->plans[p] == kPilot && p < j->next_plan) j->next_plan = p;
            ln.screen_overflowed();
        } else if (ok) {
            ln.screen_held();
        }
    }
    // (the int8 screen's suspects per query: decides whether the table's passes get the refinement stage)
    if (j->susp_stat && ok && j->stat_wide) ln.note_wide_susp((float)j->h_status[kI4mStatAt + 1] / (float)j->nq);
    if (plan == kPredict && ok && j->susp_stat &&
        (double)j->h_status[kI4mStatAt + 4] > ctx->knobs.predict_max_factor * (double)j->k * j->nq) {
        // The predicted thresholds held but admitted far more than K rows per query as CANDIDATES (exact score >= threshold): on
        // clustered rows the model's margin — a few per cent of the distance between a query's mean score and its K-th best — is
        // many times the spread of the scores inside the query's cluster, every member of which then is a true candidate (20 per
        // answer; the refinement stage cannot reject what really reaches the threshold, while the sample's threshold leaves 7-15
        // suspects of which it keeps one).  Such a table goes back to the pilot plan; the model gets another try after an
        // exponentially growing number of batches.
        ln.pred_failed(false);
        if (ctx->knobs.debug_scan) fprintf(stderr, "[pg] plan %d held with %.1f candidates per answer: pilot plan for the next %u batches\n", plan,
                                           (double)j->h_status[kI4mStatAt + 4] / j->nq / j->k, ln.pred_backoff);
    }
    if (j->susp_stat && ok) {
        ctx->stats.recall_rescored += j->h_status[kI4mStatAt + 3];
        ctx->stats.recall_suspects += j->h_status[kI4mStatAt + 1];
        ctx->stats.recall_suspect_queries += j->nq;
        ctx->stats.recall_i4m_pairs += j->h_status[kI4mStatAt];
    }
    if (j->screen4m && j->susp_stat && ok) {
        // what the 4-bit stage lets through per query decides up to which batch size it beats the int8 shadow (recall_job_prepare)
        const float per_q = (float)j->h_status[kI4mStatAt] / (float)j->nq;
        ln.note_i4m_pairs(per_q);
        if (ctx->knobs.debug_scan) fprintf(stderr, "[pg] plan %d 4-bit stage: %.0f pairs per query (running %.0f)\n", plan, per_q, ln.i4m_pairs);
    }
    if (!ok) ctx->stats.recall_rescans++;
    if (ok && plan == kPredict) ctx->stats.recall_predicted++;
    // a refined threshold that fails verification on most of a batch says the head of the table is not representative
    // (ordered rows): after two such batches the table's recalls stop refining (a hint, not state anyone relies on)
    if (!ok && (plan == kPilot || plan == kPredict) && j->refined && j->failed.size() > j->nq / 2) ln.prefix_failures++;
    *ok_out = ok;
    return PG_OK;
}

void recall_job_finish(RecallJob* j) {
    pg_ctx* ctx = j->ctx;
    ctx->stats.recall_calls++;
    ctx->stats.recall_rows_scanned += j->scanned_rows;
    if (j->timers) {                                   // (a batch without stage timers leaves the last direct call's figures)
        ctx->stats.last_recall_ms = j->total_ms;
        ctx->last_scan_ms = j->scan_ms;
    }
    ctx->last_scan_launches = j->scan_launches;
    ctx->last_scan_bytes = j->scan_bytes;              // bytes the scan launches streamed (fp32 rows, int8 / bf16 / 4-bit shadow)
}

int recall_patch_failed_locked(RecallJob* j, uint32_t* counts) {
    pg_ctx* ctx = j->ctx;
    const std::vector<uint32_t> failed = j->failed;
    RecallOpts o;
    o.skip_pilot = true;
    o.l2 = j->l2;
    o.filter = j->filter.col ? &j->filter : nullptr;
    o.exact_only = j->exact_only;
    o.no_index = j->no_index;
    for (uint32_t q : failed) {
        uint32_t cnt = 0;
        int rc;
        if ((rc = recall_dev_locked(ctx, j->t, j->d_queries + (size_t)q * j->t->dim, 1, j->k, j->d_out_rows + (size_t)q * j->k,
                                    j->d_out_scores + (size_t)q * j->k, &cnt, j->d_out_count ? j->d_out_count + q : nullptr, o)))
            return rc;
        counts[q] = cnt;
    }
    j->failed.clear();
    return PG_OK;
}

}  // namespace pg
