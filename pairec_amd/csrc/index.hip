// index.hip — an exact IVF-partitioned index over a table.
//
// Build (all on the device): k-means over a sample of the rows (Lloyd, deterministic centroid sums in fp64), every row assigned
// to its nearest centroid, a stable sort by list into a uint32 permutation (rows of one list in ascending source order) with the
// lists' offsets, a per-list radius r_L >= max ||x - c_L|| over the rows actually assigned (fp64, rounded up) and ||c_L||.
//
// Search, per batch of queries:
//   bound    U[q][L] >= every chain score of list L's rows (squared Euclidean: >= every -d), from q.c_L, ||q||, r_L and the
//            chain's rounding error (the slack derived in DESIGN.md 4.1f)
//   probe    per query, the lists of largest bound until >= K rows are covered (a weighted radix select over the bounds), scored
//            exactly: the K-th best score is thr_q, a lower bound of the final K-th best
//   scan     the lists that are not in the probe and whose bound reaches thr_q (inclusive), scored exactly; a row joins the
//            query's candidates when its score reaches the running threshold
//   select   recall_select.hip's select / final kernels: the same keys (score totalOrder descending, then row ascending) as the table pass
// Every row is scored by recall.hip's rescore_kernel — the specification's k-ascending fmaf chain — so its bits are the table
// pass's bits; pruning drops only lists whose bound proves that none of their rows can reach thr_q.
//
// One launch sequence (index_search) serves both callers.  After each stage's count a plan kernel writes the verdict — the dense
// rule, a non-finite query, the rounds the stage takes — into the plan words, and every round's expansion reads it.  The two
// callers differ only in their round policy:
//   pg_index_recall_topk*   the host reads the words after each stage, falls back to the table's pass on a flag, and runs exactly
//                           the rounds counted (no budget)
//   an attached index       (pg_index_attach) a RecallJob plan that is only enqueued: index_plan_rounds rounds per
//                           stage, rounds past the verdict's do nothing; recall_job_check reads the words with the job's status
//                           words and moves to the table's own plans when a flag is set
#include "common.hpp"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <list>

namespace pg {
// an attached index's serving counters and its switch, shared with the jobs that tried it (a job's check may come after a
// detach and destroy: the jobs keep this alive, not the index)
constexpr int kBands = 5;                  // batch sizes 1, 2-8, 9-32, 33-64, 65-256
struct IndexServe {
    std::atomic<uint64_t> plans{0}, plans_held{0}, queries_held{0};
    std::atomic<uint64_t> replan_dense{0}, replan_rounds{0}, replan_overflow{0}, replan_nonfinite{0};
    std::atomic<uint64_t> skipped_stale{0}, skipped_switch{0};
    std::atomic<uint64_t> queries{0}, pairs{0}, rows_live{0}, max_scan{0};
    std::atomic<int32_t> skip[kBands] = {};   // batches of the band that skip the index plan before it is tried again
};

// The lists of an index restricted to the rows a filter admits: list L holds perm[off[L], off[L + 1]), the
// index's rows of L that pass, in the same (ascending source) order.  One allocation, freed with the last reference: a call that
// searches an entry holds it until its stream has synchronised, so an eviction by another context never frees it under a search.
struct WhereKey {
    const pg_features* fs;
    int column;
    uint64_t version;                    // the column's (process-wide counter: a rewritten or reallocated column never matches)
    int op;
    long long value;
    uint64_t gen;                        // the index's table generation
    // a compound clause: its identity and its bitmap's epoch (column -1; version, op and value 0) — a bitmap
    // rebuilt after a column changed has a new epoch, and no two builds in a process share one
    const pg_where* w;
    uint64_t epoch;
    bool operator==(const WhereKey& o) const {
        return fs == o.fs && column == o.column && version == o.version && op == o.op && value == o.value && gen == o.gen && w == o.w &&
               epoch == o.epoch;
    }
};
struct WhereLists {
    WhereKey key{};
    void* d = nullptr;
    uint32_t* off = nullptr;             // [n_lists + 1]
    uint32_t* perm = nullptr;            // [admitted]
    uint64_t admitted = 0;
    size_t bytes = 0;                    // admitted x 4 + (n_lists + 1) x 4 (the offsets padded to 256 B)
    ~WhereLists() { if (d) (void)hipFree(d); }
};
}  // namespace pg

struct pg_index {
    const pg_table* t = nullptr;
    uint64_t gen = 0;
    uint64_t rows = 0;
    uint32_t dim = 0, n_lists = 0;
    bool nonfinite = false;
    uint32_t* d_perm = nullptr;   // [rows] source rows, list by list
    uint32_t* d_off = nullptr;    // [n_lists + 1] list offsets into d_perm
    float* d_cent = nullptr;      // [n_lists][dim] centroids
    float* d_cnorm = nullptr;     // [n_lists] ||c_L||, rounded up
    float* d_rad = nullptr;       // [n_lists] r_L, rounded up
    void* d_small = nullptr;      // the allocation behind d_off / d_cent / d_cnorm / d_rad
    std::mutex mu;                // guards st
    pg_index_stats_t st{};        // the synchronous pg_index_recall_topk* calls (the attached plans count in serve)
    std::shared_ptr<pg::IndexServe> serve = std::make_shared<pg::IndexServe>();
    // filtered lists: at most "index_where_cache" entries, most recently used first.  where_mu is taken after
    // ctx->mu and the table's shared lock; it also guards where_st.
    std::mutex where_mu;
    std::list<std::shared_ptr<pg::WhereLists>> where_cache;
    pg_index_where_stats_t where_st{};
    // pg_index_refresh: one refresh of an index at a time (taken after ctx->mu, before the table's lock); the
    // counters are guarded by mu
    std::mutex refresh_mu;
    pg_index_refresh_stats_t rst{};
};

namespace pg {
namespace {

constexpr uint32_t kMaxLists = 65536;
constexpr uint32_t kSlices = 256;        // list slices of the count / expand kernels (per query)
constexpr uint32_t kBoundQ = 8;          // queries per bound-kernel block
// the dense rule of a filter's lists: the filtered pass costs about as much as the table's pass (rows) or, when
// it gathers a compact copy, this many table-pass rows per admitted row (profiles/index_where.json: the breakevens at 0.1 % and
// 1 % admitted put it at ~140 and ~80)
constexpr double kWhereGatherWeight = 150.0;

// the verdict of an index plan, written by the device (index_plan_kernel) and read by every later launch of the plan, then
// copied into the job's status words at kIndexStatAt
struct IndexPlanWords {
    uint32_t flags;                      // kPlanNonfinite | kPlanDense | kPlanRounds: the table's plans serve the batch
    uint32_t need[2];                    // rounds the probe (0) and the scan (1) take
    uint32_t max_probe;                  // the most rows one query's probe scores
    unsigned long long pairs[2];         // (row, query) pairs of the probe and the scan
    unsigned long long union_rows;       // rows of the lists live for some query (union_kernel)
    unsigned long long max_scan;         // the most rows one query's scan scores
};
static_assert(sizeof(IndexPlanWords) == 48, "12 status words");
constexpr uint32_t kPlanNonfinite = 1u, kPlanDense = 2u, kPlanRounds = 4u;

__device__ __forceinline__ uint32_t ukey(float f) {      // order-preserving bits (totalOrder for non-NaN)
    const uint32_t b = __float_as_uint(f);
    if (f != f) return 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the smallest float >= v
__device__ __forceinline__ float round_up_f(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, __builtin_inff());
    return f;
}

// ---- build ---------------------------------------------------------------------------------------------------
__global__ void sample_gather_kernel(const float* __restrict__ tab, uint64_t rows, uint32_t dim, uint64_t mul, uint64_t add,
                                     float* __restrict__ out) {
    const uint64_t i = blockIdx.x;
    const uint64_t r = (mul * i + add) % rows;               // mul coprime to rows: distinct rows for i < rows
    for (uint32_t c = threadIdx.x; c < dim; c += blockDim.x) out[i * dim + c] = tab[r * dim + c];
}

__global__ void iota_kernel(uint32_t* __restrict__ v, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

__global__ void cnorm2_kernel(const float* __restrict__ c, uint32_t nl, uint32_t dim, float* __restrict__ out) {
    const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= nl) return;
    float s = 0.0f;
    for (uint32_t k = 0; k < dim; ++k) s = __fmaf_rn(c[(size_t)L * dim + k], c[(size_t)L * dim + k], s);
    out[L] = s;
}

// nearest centroid (smallest ||c||^2 - 2 x.c, ties to the lower list) of rows [0, n) of X: 64 rows x 64 centroids per step, every
// thread 4 x 4 of them.  Only speed depends on this arithmetic: the radius is measured over the assignment it makes.
template <int DIM>
__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ X, uint64_t n, const float* __restrict__ C,
                                                     const float* __restrict__ cn2, uint32_t nl, uint32_t* __restrict__ out,
                                                     uint32_t* __restrict__ nonfinite) {
    extern __shared__ float sm[];
    float* const Xs = sm;                    // [DIM][65]
    float* const Cs = sm + DIM * 65;         // [DIM][65]
    const uint64_t r0 = (uint64_t)blockIdx.x * 64;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    bool bad = false;
    for (int e = tid; e < 64 * DIM; e += 256) {
        const int r = e / DIM, c = e % DIM;
        const float v = r0 + r < n ? X[(r0 + r) * DIM + c] : 0.0f;
        bad |= !isfinite(v);
        Xs[c * 65 + r] = v;
    }
    if (bad) atomicOr(nonfinite, 1u);
    float best[4];
    uint32_t bi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = __builtin_inff(); bi[i] = 0xFFFFFFFFu; }
    for (uint32_t c0 = 0; c0 < nl; c0 += 64) {
        __syncthreads();
        for (int e = tid; e < 64 * DIM; e += 256) {
            const int cc = e / DIM, c = e % DIM;
            Cs[c * 65 + cc] = c0 + cc < nl ? C[(size_t)(c0 + cc) * DIM + c] : 0.0f;
        }
        __syncthreads();
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
        for (int k = 0; k < DIM; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = Xs[k * 65 + ty + 16 * i]; b[i] = Cs[k * 65 + tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __fmaf_rn(a[i], b[j], acc[i][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t ci = c0 + tx + 16 * j;
            if (ci >= nl) continue;
            const float cc = cn2[ci];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = cc - 2.0f * acc[i][j];
                if (d < best[i]) { best[i] = d; bi[i] = ci; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        for (int off = 8; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best[i], off);
            const uint32_t oi = (uint32_t)__shfl_xor((int)bi[i], off);
            if (ob < best[i] || (ob == best[i] && oi < bi[i])) { best[i] = ob; bi[i] = oi; }
        }
        const uint64_t r = r0 + ty + 16 * i;
        if (tx == 0 && r < n) out[r] = bi[i] < nl ? bi[i] : 0u;      // (a NaN row: list 0)
    }
}

// offsets of a sorted key array: off[L] = first position whose key is >= L, off[nl] = n
__global__ void list_offsets_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint32_t nl, uint32_t* __restrict__ off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const uint32_t lo = i == 0 ? 0u : keys[i - 1] + 1u;
    const uint32_t hi = i == n ? nl : keys[i];
    for (uint32_t L = lo; L <= hi && L <= nl; ++L) off[L] = (uint32_t)i;
}

// Lloyd update: centroid L = mean of its sample rows (summed in fp64, in sorted order: deterministic); an empty list is re-seeded
// with a sample row
__global__ void centroid_update_kernel(const float* __restrict__ S, uint32_t n_sample, uint32_t dim, const uint32_t* __restrict__ sorted_idx,
                                       const uint32_t* __restrict__ off, float* __restrict__ C, uint64_t salt) {
    const uint32_t L = blockIdx.x;
    const uint32_t b = off[L], e = off[L + 1];
    if (b == e) {
        const uint32_t r = (uint32_t)((((uint64_t)L + 1) * 0x9E3779B97F4A7C15ull + salt) % n_sample);
        for (uint32_t c = threadIdx.x; c < dim; c += blockDim.x) C[(size_t)L * dim + c] = S[(size_t)r * dim + c];
        return;
    }
    for (uint32_t c = threadIdx.x; c < dim; c += blockDim.x) {
        double s = 0.0;
        for (uint32_t j = b; j < e; ++j) s += (double)S[(size_t)sorted_idx[j] * dim + c];
        C[(size_t)L * dim + c] = (float)(s / (double)(e - b));
    }
}

// r_L >= max ||x - c_L|| over the rows assigned to L: fp64 distances, a relative margin for their rounding, rounded up to fp32
__global__ void radius_kernel(const float* __restrict__ tab, uint64_t rows, uint32_t dim, const uint32_t* __restrict__ assign,
                              const float* __restrict__ C, uint32_t* __restrict__ rad_bits) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint32_t L = assign[i];
    double s = 0.0;
    for (uint32_t k = 0; k < dim; ++k) {
        const double d = (double)tab[i * dim + k] - (double)C[(size_t)L * dim + k];
        s = fma(d, d, s);
    }
    const float r = round_up_f(sqrt(s) * (1.0 + 0x1p-40));
    atomicMax(&rad_bits[L], __float_as_uint(r));             // (non-negative floats order as their bits)
}

__global__ void cnorm_kernel(const float* __restrict__ C, uint32_t nl, uint32_t dim, float* __restrict__ out) {
    const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= nl) return;
    double s = 0.0;
    for (uint32_t k = 0; k < dim; ++k) s = fma((double)C[(size_t)L * dim + k], (double)C[(size_t)L * dim + k], s);
    out[L] = round_up_f(sqrt(s) * (1.0 + 0x1p-40));
}

// ---- refresh ----------------------------------------------------------------------------------
// the per-row list recovered from the index: position p of the permutation lies in list L with off[L] <= p < off[L + 1]
__global__ void list_of_row_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off, uint64_t rows, uint32_t nl,
                                   uint32_t* __restrict__ assign) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= rows) return;
    uint32_t lo = 0, hi = nl;                // the last L with off[L] <= p (off[0] = 0, off[nl] = rows > p)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= (uint32_t)p) lo = mid;
        else hi = mid;
    }
    const uint32_t row = perm[p];
    if (row < rows) assign[row] = lo;
}

__global__ void iota_from_kernel(uint32_t* __restrict__ v, uint64_t n, uint32_t first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = first + (uint32_t)i;
}

// assign[ids[i]] = vals[i]; moved (may be null: assign holds nothing to compare with) += the rows whose list changes
__global__ void patch_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ vals, uint32_t n, uint64_t rows,
                             uint32_t* __restrict__ assign, unsigned long long* __restrict__ moved) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool m = false;
    if (i < n && ids[i] < rows) {
        m = moved && assign[ids[i]] != vals[i];
        assign[ids[i]] = vals[i];
    }
    if (!moved) return;                      // (uniform)
    const unsigned long long c = __popcll(__builtin_amdgcn_ballot_w64(m));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(moved, c);
}

__global__ void count_moved_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t rows,
                                   unsigned long long* __restrict__ moved) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool m = i < rows && a[i] != b[i];
    const unsigned long long c = __popcll(__builtin_amdgcn_ballot_w64(m));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(moved, c);
}

// *flag |= 1 when an element of the table is not finite
__global__ void finite_kernel(const float* __restrict__ tab, uint64_t n_elems, uint32_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_elems; i += stride) bad |= !isfinite(tab[i]);
    if (bad) atomicOr(flag, 1u);
}

// ---- search --------------------------------------------------------------------------------------------------
// per query: an upper bound of ||q|| (fp64) and whether every element is finite
__global__ void qinfo_kernel(const float* __restrict__ Q, uint32_t dim, double* __restrict__ qn, uint32_t* __restrict__ flag) {
    const uint32_t q = blockIdx.x;
    double s = 0.0;
    bool bad = false;
    for (uint32_t c = threadIdx.x; c < dim; c += 64) {
        const float v = Q[(size_t)q * dim + c];
        bad |= !isfinite(v);
        s = fma((double)v, (double)v, s);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (bad) atomicOr(flag, 1u);
    if (threadIdx.x == 0) qn[q] = sqrt(s) * (1.0 + 0x1p-40);
}

// U[q][L].  Inner product: fl(x.q) <= q.c + r ||q|| + gamma_d (||c|| + r) ||q|| (+ underflow and fp64 terms).
// Squared Euclidean (ranked by -d): -fl(d) <= -(max(0, ||q - c|| - r))^2 + gamma_{d+3} (||c|| + r + ||q||)^2 (+ the same).
// Where a partial sum could overflow fp32 the bound is +inf (the list is always scanned).
template <bool L2>
__global__ __launch_bounds__(256) void bound_kernel(const float* __restrict__ Q, uint32_t nq, uint32_t dim, const double* __restrict__ qn,
                                                    const float* __restrict__ C, const float* __restrict__ cnorm, const float* __restrict__ rad,
                                                    uint32_t nl, float* __restrict__ U) {
    extern __shared__ double qs[];           // [kBoundQ][dim]
    const uint32_t q0 = blockIdx.y * kBoundQ;
    for (uint32_t e = threadIdx.x; e < kBoundQ * dim; e += blockDim.x) {
        const uint32_t j = e / dim, c = e % dim;
        qs[e] = q0 + j < nq ? (double)Q[(size_t)(q0 + j) * dim + c] : 0.0;
    }
    __syncthreads();
    const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= nl) return;
    double acc[kBoundQ];
#pragma unroll
    for (int j = 0; j < (int)kBoundQ; ++j) acc[j] = 0.0;
    for (uint32_t c = 0; c < dim; ++c) {
        const double cv = (double)C[(size_t)L * dim + c];
#pragma unroll
        for (int j = 0; j < (int)kBoundQ; ++j) {
            if (L2) {
                const double d = qs[j * dim + c] - cv;
                acc[j] = fma(d, d, acc[j]);
            } else {
                acc[j] = fma(cv, qs[j * dim + c], acc[j]);
            }
        }
    }
    const double u = 0x1p-24;
    const double dd = (double)dim + (L2 ? 3.0 : 0.0);
    const double gam = dd * u / (1.0 - dd * u);
    const double r = (double)rad[L], cn = (double)cnorm[L];
#pragma unroll
    for (int j = 0; j < (int)kBoundQ; ++j) {
        const uint32_t q = q0 + j;
        if (q >= nq) break;
        const double qv = qn[q];
        float out;
        if (L2) {
            const double b = cn + r + qv;
            if (!(b * b * 2.0 < 0x1p126)) {
                out = __builtin_inff();
            } else {
                const double s = sqrt(acc[j]) * (1.0 - 0x1p-40);
                const double lb = s > r ? s - r : 0.0;
                const double lb2 = lb * lb * (1.0 - 0x1p-40);
                const double err = gam * b * b * (1.0 + 0x1p-20) + 0x1p-40 * b * b + (double)dim * 0x1p-146;
                out = round_up_f(err - lb2);
            }
        } else {
            const double a = (cn + r) * qv;
            if (!(a * (1.0 + gam) * 2.0 < 0x1p127)) {
                out = __builtin_inff();
            } else {
                const double slack = gam * a * (1.0 + 0x1p-20) + 0x1p-40 * a + (double)dim * 0x1p-148;
                out = round_up_f(acc[j] + r * qv + slack);
            }
        }
        U[(size_t)q * nl + L] = out;
    }
}

// per query: the largest bound key B with sum(size of lists with key >= B) >= K (a radix select weighted by list size); the
// probe is those lists, probe_rows[q] their rows.  A table of <= K rows probes everything (B = 0).
__global__ __launch_bounds__(1024) void probe_kernel(const float* __restrict__ U, uint32_t nl, const uint32_t* __restrict__ off,
                                                     uint64_t rows, uint32_t K, uint32_t* __restrict__ Bkey, uint32_t* __restrict__ probe_rows) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_digit, s_need;
    __shared__ unsigned long long s_tot;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const float* u = U + (size_t)q * nl;
    uint32_t prefix = 0, mask = 0, need = K;
    if (rows > K) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (uint32_t L = tid; L < nl; L += 1024) {
                const uint32_t sz = off[L + 1] - off[L];
                const uint32_t key = ukey(u[L]);
                if (sz && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], sz);
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t above = 0;
                for (int d = 255; d > (int)tid; --d) above += hist[d];
                if (above < need && need <= above + hist[tid]) { s_digit = tid; s_need = need - above; }
            }
            __syncthreads();
            prefix |= s_digit << shift;
            mask |= 255u << shift;
            need = s_need;
            __syncthreads();
        }
    }
    if (tid == 0) s_tot = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint32_t L = tid; L < nl; L += 1024)
        if (ukey(u[L]) >= prefix) mine += off[L + 1] - off[L];
    atomicAdd(&s_tot, mine);
    __syncthreads();
    if (tid == 0) {
        Bkey[q] = prefix;
        probe_rows[q] = (uint32_t)s_tot;
    }
}

// mode 0 (probe): key(U) >= B;  mode 1 (scan): U reaches thr (inclusive; a NaN threshold admits everything) and key(U) < B
__device__ __forceinline__ bool list_selected(int mode, float u, uint32_t B, float thr) {
    const uint32_t key = ukey(u);
    return mode == 0 ? key >= B : (!(u < thr) && key < B);
}

__device__ __forceinline__ void slice_of(uint32_t nl, uint32_t g, uint32_t& lo, uint32_t& hi) {
    const uint32_t per = (nl + kSlices - 1) / kSlices;
    lo = g * per < nl ? g * per : nl;
    hi = lo + per < nl ? lo + per : nl;
}

// rows of the selected lists per (query, slice)
__global__ __launch_bounds__(256) void count_kernel(const float* __restrict__ U, uint32_t nl, const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ Bkey, const float* __restrict__ thr, int mode,
                                                    uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wsum[4];
    const uint32_t q = blockIdx.y, g = blockIdx.x;
    uint32_t lo, hi;
    slice_of(nl, g, lo, hi);
    const float* u = U + (size_t)q * nl;
    const uint32_t B = Bkey[q];
    const float th = thr[q];
    uint32_t s = 0;
    for (uint32_t L = lo + threadIdx.x; L < hi; L += 256)
        if (list_selected(mode, u[L], B, th)) s += off[L + 1] - off[L];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(size_t)q * kSlices + g] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// the rows of the selected lists, in (slice, list) order, positions [round x scap, (round + 1) x scap) of that sequence →
// susp[q][0, scap).  pw (an index plan): nothing to do once a flag is set or past the rounds the plan kernel counted — the round's
// suspect lists are left empty, so its re-scoring returns at once.
__global__ __launch_bounds__(256) void expand_kernel(const float* __restrict__ U, uint32_t nl, const uint32_t* __restrict__ off,
                                                     const uint32_t* __restrict__ perm, const uint32_t* __restrict__ Bkey,
                                                     const float* __restrict__ thr, int mode, const uint32_t* __restrict__ cnt,
                                                     uint32_t round, uint32_t scap, uint32_t* __restrict__ susp,
                                                     uint32_t* __restrict__ susp_cnt, const IndexPlanWords* __restrict__ pw) {
    __shared__ uint32_t sc[256];
    __shared__ uint32_t e_start[256], e_len[256];
    __shared__ long long e_dst[256];
    __shared__ uint32_t s_n;
    __shared__ long long s_base;
    const uint32_t q = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    if (pw && (pw->flags != 0u || round >= pw->need[mode])) {        // (the same for the whole block)
        if (g == 0 && tid == 0) susp_cnt[q] = 0u;
        return;
    }
    const uint64_t skip = (uint64_t)round * scap;
    if (tid == 0) {
        unsigned long long before = 0, total = 0;
        for (uint32_t i = 0; i < kSlices; ++i) {
            const uint32_t c = cnt[(size_t)q * kSlices + i];
            if (i < g) before += c;
            total += c;
        }
        s_base = (long long)before - (long long)skip;
        s_n = 0;
        if (g == 0) {
            const long long rem = (long long)total - (long long)skip;
            susp_cnt[q] = rem <= 0 ? 0u : (rem < (long long)scap ? (uint32_t)rem : scap);
        }
    }
    __syncthreads();
    uint32_t lo, hi;
    slice_of(nl, g, lo, hi);
    const float* u = U + (size_t)q * nl;
    const uint32_t B = Bkey[q];
    const float th = thr[q];
    uint32_t* const out = susp + (size_t)q * scap;
    long long base = s_base;
    for (uint32_t c0 = lo; c0 < hi; c0 += 256) {
        const uint32_t L = c0 + tid;
        const bool sel = L < hi && list_selected(mode, u[L], B, th);
        const uint32_t b = sel ? off[L] : 0u;
        const uint32_t sz = sel ? off[L + 1] - b : 0u;
        sc[tid] = sz;
        __syncthreads();
        for (uint32_t o = 1; o < 256; o <<= 1) {            // inclusive scan of the sizes
            const uint32_t v = tid >= o ? sc[tid - o] : 0u;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const long long dst = base + (long long)(sc[tid] - sz);
        if (sz && dst < (long long)scap && dst + (long long)sz > 0) {
            const uint32_t e = atomicAdd(&s_n, 1u);
            e_start[e] = b;
            e_len[e] = sz;
            e_dst[e] = dst;
        }
        const uint32_t chunk = sc[255];
        __syncthreads();
        const uint32_t n_e = s_n;
        for (uint32_t e = 0; e < n_e; ++e) {
            const uint32_t st = e_start[e], len = e_len[e];
            const long long d0 = e_dst[e];
            for (uint32_t j = tid; j < len; j += 256) {
                const long long p = d0 + (long long)j;
                if (p >= 0 && p < (long long)scap) out[p] = perm[st + j];
            }
        }
        base += chunk;
        __syncthreads();
        if (tid == 0) s_n = 0;
        __syncthreads();
    }
}

// rows of the lists that are live for at least one query of the batch (probe or scan): what a scan that loads every live list
// once for all its queries would read
__global__ __launch_bounds__(256) void union_kernel(const float* __restrict__ U, uint32_t nl, uint32_t nq, const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ Bkey, const float* __restrict__ thr,
                                                    unsigned long long* __restrict__ out) {
    const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long s = 0;
    if (L < nl) {
        bool live = false;
        for (uint32_t q = 0; q < nq && !live; ++q) {
            const float u = U[(size_t)q * nl + L];
            live = list_selected(0, u, Bkey[q], thr[q]) || list_selected(1, u, Bkey[q], thr[q]);
        }
        if (live) s = off[L + 1] - off[L];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

// a search's start: thresholds -inf, candidate counts and the overflow word 0, the plan's words cleared
__global__ void index_plan_init_kernel(float* __restrict__ thr, uint32_t* __restrict__ cnt, uint32_t* __restrict__ overflow,
                                       IndexPlanWords* __restrict__ pw) {
    const uint32_t i = threadIdx.x;
    thr[i] = -__builtin_inff();
    cnt[i] = 0u;
    if (i == 0) *overflow = 0u;
    if (i < sizeof(IndexPlanWords) / 4) reinterpret_cast<uint32_t*>(pw)[i] = 0u;
}

// a stage's verdict (launched <<<1, kMaxQueries>>> after the count of `mode`): the (row, query) pairs of the batch, the dense
// rule against `limit` (the probe's pairs, then probe + scan), the most rows one query scores and the rounds of scap suspects
// that takes — more than `budget` of them is a flag too
__global__ __launch_bounds__(256) void index_plan_kernel(const uint32_t* __restrict__ cnt, uint32_t nq, int mode, uint32_t scap,
                                                         uint32_t budget, double limit, IndexPlanWords* __restrict__ pw) {
    __shared__ unsigned long long s_tot[4], s_max[4];
    const uint32_t q = threadIdx.x;
    unsigned long long v = 0;
    if (q < nq)
        for (uint32_t g = 0; g < kSlices; ++g) v += cnt[(size_t)q * kSlices + g];
    unsigned long long tot = v, mx = v;
    for (int o = 32; o > 0; o >>= 1) {
        tot += __shfl_xor(tot, o);
        const unsigned long long om = __shfl_xor(mx, o);
        mx = om > mx ? om : mx;
    }
    if ((q & 63) == 0) { s_tot[q >> 6] = tot; s_max[q >> 6] = mx; }
    __syncthreads();
    if (q != 0) return;
    tot = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
    mx = s_max[0];
    for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
    const unsigned long long need = (mx + scap - 1) / scap;
    uint32_t f = 0;
    if ((double)(mode == 0 ? tot : pw->pairs[0] + tot) > limit) f |= kPlanDense;
    if (need > budget) f |= kPlanRounds;
    pw->pairs[mode] = tot;
    pw->need[mode] = (uint32_t)(need < budget ? need : budget);
    if (mode == 0) pw->max_probe = (uint32_t)mx;
    else pw->max_scan = mx;
    if (f) pw->flags |= f;
}

// the status block of an index plan (<<<1, kMaxQueries>>>): [0] the re-scoring's overflow flag, [1 + q] valid counts (as every
// plan's), [kIndexStatAt, + 12) the plan's words
__global__ void index_status_kernel(const uint32_t* __restrict__ overflow, uint32_t nq, const IndexPlanWords* __restrict__ pw,
                                    uint32_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    out[1 + t] = t < nq ? overflow[1 + t] : 0u;
    if (t < sizeof(IndexPlanWords) / 4) out[kIndexStatAt + t] = reinterpret_cast<const uint32_t*>(pw)[t];
    if (t == 0) out[0] = overflow[0];
}

// ---- filtered lists -------------------------------------------------------------------------
// bit r of bits: row r passes the filter.  Rows in order (the column is read coalesced); a wave's 64 rows are two words.
__global__ __launch_bounds__(256) void where_bits_kernel(RowFilter f, uint64_t rows, uint32_t* __restrict__ bits) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool pass = r < rows && row_filter_pass(f, (uint32_t)r);
    const uint64_t m = __builtin_amdgcn_ballot_w64(pass);
    if ((threadIdx.x & 63) == 0 && r < rows) {
        bits[r >> 5] = (uint32_t)m;
        if (r + 32 < rows) bits[(r >> 5) + 1] = (uint32_t)(m >> 32);
    }
}

// one block per list: the positions of list L whose row passes (bits[perm[p]], a gather from a bitmap of rows / 8 bytes).
// COUNT: cnt[L] = how many.  Else the stable compaction: perm_f[off_f[L] + rank] = perm[p], ranks in position order.
template <bool COUNT>
__global__ __launch_bounds__(256) void where_lists_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt_off,
                                                          uint32_t* __restrict__ perm_f) {
    __shared__ uint32_t wsum[4];
    const uint32_t L = blockIdx.x;
    const uint32_t b = off[L], e = off[L + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t base = COUNT ? 0u : cnt_off[L];
    for (uint32_t p0 = b; p0 < e; p0 += 256) {
        const uint32_t p = p0 + threadIdx.x;
        const uint32_t row = p < e ? perm[p] : 0u;
        const bool pass = p < e && ((bits[row >> 5] >> (row & 31)) & 1u);
        const uint64_t m = __builtin_amdgcn_ballot_w64(pass);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        if (!COUNT && pass) {
            uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            for (int j = 0; j < w; ++j) pos += wsum[j];
            perm_f[pos] = row;
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (COUNT && threadIdx.x == 0) cnt_off[L] = base;
}

// ---- host ----------------------------------------------------------------------------------------------------
// device allocation that reports failure as PG_ERR_NOMEM (and clears the runtime's last error)
int dalloc(void** p, size_t bytes, std::vector<void*>& owned) {
    if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return PG_ERR_NOMEM;
    }
    owned.push_back(*p);
    return PG_OK;
}

void free_all(std::vector<void*>& owned) {
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
}

template <int DIM>
int assign_launch(pg_ctx* ctx, const float* X, uint64_t n, const float* C, const float* cn2, uint32_t nl, uint32_t* out, uint32_t* flag) {
    const size_t lds = (size_t)2 * DIM * 65 * 4;
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)assign_kernel<DIM>, lds))) return rc;
    assign_kernel<DIM><<<(uint32_t)((n + 63) / 64), 256, lds, ctx->stream>>>(X, n, C, cn2, nl, out, flag);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int assign_dispatch(pg_ctx* ctx, uint32_t dim, const float* X, uint64_t n, const float* C, const float* cn2, uint32_t nl, uint32_t* out,
                    uint32_t* flag) {
    cnorm2_kernel<<<(nl + 255) / 256, 256, 0, ctx->stream>>>(C, nl, dim, const_cast<float*>(cn2));
    PG_HIP(hipGetLastError());
    switch (dim) {
        case 64: return assign_launch<64>(ctx, X, n, C, cn2, nl, out, flag);
        case 128: return assign_launch<128>(ctx, X, n, C, cn2, nl, out, flag);
        case 192: return assign_launch<192>(ctx, X, n, C, cn2, nl, out, flag);
        case 256: return assign_launch<256>(ctx, X, n, C, cn2, nl, out, flag);
    }
    set_error("pg_index_build: dim=%u unsupported", dim);
    return PG_ERR_UNSUPPORTED;
}

// stable sort of keys (list ids) with their positions: sorted keys, positions in source order within a key, offsets
int sort_end_bit(uint32_t nl) {
    int end_bit = 1;
    while (end_bit < 32 && (1ull << end_bit) < (uint64_t)nl) ++end_bit;
    return end_bit;
}

// temp storage of the largest sort of a build (hipcub's radix sort; the item count is 64-bit)
int sort_temp_bytes(uint64_t n, uint32_t nl, size_t* out) {
    *out = 0;
    PG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, *out, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                              (uint32_t*)nullptr, n, 0, sort_end_bit(nl), (hipStream_t)0));
    return PG_OK;
}

// (tmp: sort_temp_bytes of the build's largest n, allocated once)
int sort_by_list(pg_ctx* ctx, const uint32_t* keys, uint64_t n, uint32_t nl, uint32_t* keys_out, uint32_t* vals_in, uint32_t* vals_out,
                 uint32_t* off, void* tmp, size_t tmp_bytes) {
    iota_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, ctx->stream>>>(vals_in, n);
    PG_HIP(hipGetLastError());
    PG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, keys_out, vals_in, vals_out, n, 0, sort_end_bit(nl), ctx->stream));
    list_offsets_kernel<<<(uint32_t)((n + 1 + 255) / 256), 256, 0, ctx->stream>>>(keys_out, n, nl, off);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

uint64_t gcd64(uint64_t a, uint64_t b) {
    while (b) { const uint64_t t = a % b; a = b; b = t; }
    return a;
}

uint64_t splitmix(uint64_t& x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the lists' figures of pg_index_stats from their radii and offsets (the build's and every refresh's)
void list_summary(const std::vector<float>& rad, const std::vector<uint32_t>& off, pg_index_stats_t* st) {
    const uint32_t nl = (uint32_t)rad.size();
    double sum_r = 0.0;
    float max_r = 0.0f;
    uint32_t largest = 0, empty = 0;
    for (uint32_t L = 0; L < nl; ++L) {
        const uint32_t sz = off[L + 1] - off[L];
        if (!sz) { ++empty; continue; }
        largest = std::max(largest, sz);
        sum_r += rad[L];
        max_r = std::max(max_r, rad[L]);
    }
    st->max_radius = max_r;
    st->mean_radius = nl > empty ? (float)(sum_r / (nl - empty)) : 0.0f;
    st->largest_list = largest;
    st->empty_lists = empty;
}

int index_build_locked(pg_ctx* ctx, const pg_table* t, const pg_index_params& p, pg_index* ix, std::vector<void*>& owned,
                       std::vector<void*>& temp) {
    const uint64_t rows = t->rows;
    const uint32_t dim = t->dim;
    uint32_t nl = p.n_lists;
    if (nl == 0) nl = (uint32_t)std::llround(4.0 * std::sqrt((double)rows));
    if (nl > kMaxLists) nl = kMaxLists;
    if (nl > rows / 64) nl = (uint32_t)(rows / 64);
    if (nl < 1) nl = 1;
    uint64_t ns = p.train_rows ? p.train_rows : std::min<uint64_t>(rows, 64ull * nl);
    if (ns > rows) ns = rows;
    if (ns < nl) ns = nl;
    const uint32_t iters = p.iters ? p.iters : 8;
    ix->n_lists = nl;
    int rc;
    // index memory: the permutation and the per-list arrays (one allocation)
    if ((rc = dalloc((void**)&ix->d_perm, rows * 4, owned))) return rc;
    const size_t off_b = align_up((size_t)(nl + 1) * 4), cent_b = (size_t)nl * dim * 4, lists_b = align_up((size_t)nl * 4);
    if ((rc = dalloc(&ix->d_small, off_b + cent_b + 2 * lists_b, owned))) return rc;
    ix->d_off = (uint32_t*)ix->d_small;
    ix->d_cent = (float*)((char*)ix->d_small + off_b);
    ix->d_cnorm = (float*)((char*)ix->d_cent + cent_b);
    ix->d_rad = (float*)((char*)ix->d_cnorm + lists_b);
    // build temporaries
    float *S, *cn2;
    uint32_t *assign, *keys_s, *vals_in, *vals_s, *soff, *flag;
    if ((rc = dalloc((void**)&S, ns * dim * 4, temp))) return rc;
    if ((rc = dalloc((void**)&cn2, (size_t)nl * 4, temp))) return rc;
    if ((rc = dalloc((void**)&assign, rows * 4, temp))) return rc;
    if ((rc = dalloc((void**)&keys_s, rows * 4, temp))) return rc;
    if ((rc = dalloc((void**)&vals_in, rows * 4, temp))) return rc;
    if ((rc = dalloc((void**)&soff, ((size_t)nl + 1) * 4, temp))) return rc;
    if ((rc = dalloc((void**)&flag, 16, temp))) return rc;
    size_t tmp_bytes = 0, tmp_small = 0;
    void* tmp;
    if ((rc = sort_temp_bytes(rows, nl, &tmp_bytes)) || (rc = sort_temp_bytes(ns, nl, &tmp_small))) return rc;
    tmp_bytes = std::max(tmp_bytes, tmp_small);
    if ((rc = dalloc(&tmp, tmp_bytes, temp))) return rc;
    vals_s = ix->d_perm;                     // (the sample's sort uses the permutation's memory before the table's does)
    PG_HIP(hipMemsetAsync(flag, 0, 16, ctx->stream));
    // 1. the sample: rows (mul * i + add) mod rows, mul coprime to rows; the first n_lists of them seed the centroids
    uint64_t sx = p.seed ^ 0x1D8E4E27C47D124Full;
    uint64_t mul = rows > 1 ? 1 + splitmix(sx) % (rows - 1) : 1;
    while (gcd64(mul, rows) != 1) mul = mul + 1 < rows ? mul + 1 : 1;
    const uint64_t add = splitmix(sx) % rows;
    sample_gather_kernel<<<(uint32_t)ns, 64, 0, ctx->stream>>>(t->d, rows, dim, mul, add, S);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(ix->d_cent, S, (size_t)nl * dim * 4, hipMemcpyDeviceToDevice, ctx->stream));
    // 2. Lloyd iterations over the sample
    for (uint32_t it = 0; it < iters; ++it) {
        if ((rc = assign_dispatch(ctx, dim, S, ns, ix->d_cent, cn2, nl, assign, flag + 1))) return rc;
        if ((rc = sort_by_list(ctx, assign, ns, nl, keys_s, vals_in, vals_s, soff, tmp, tmp_bytes))) return rc;
        centroid_update_kernel<<<nl, 64, 0, ctx->stream>>>(S, (uint32_t)ns, dim, vals_s, soff, ix->d_cent, splitmix(sx));
        PG_HIP(hipGetLastError());
    }
    // 3. every row to its nearest centroid; the stable sort by list is the permutation
    if ((rc = assign_dispatch(ctx, dim, t->d, rows, ix->d_cent, cn2, nl, assign, flag))) return rc;
    if ((rc = sort_by_list(ctx, assign, rows, nl, keys_s, vals_in, ix->d_perm, ix->d_off, tmp, tmp_bytes))) return rc;
    // 4. radii over the rows actually assigned, 5. centroid norms
    PG_HIP(hipMemsetAsync(ix->d_rad, 0, (size_t)nl * 4, ctx->stream));
    radius_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, ctx->stream>>>(t->d, rows, dim, assign, ix->d_cent, (uint32_t*)ix->d_rad);
    PG_HIP(hipGetLastError());
    cnorm_kernel<<<(nl + 255) / 256, 256, 0, ctx->stream>>>(ix->d_cent, nl, dim, ix->d_cnorm);
    PG_HIP(hipGetLastError());
    std::vector<float> rad(nl);
    std::vector<uint32_t> off(nl + 1);
    uint32_t h_flag = 0;
    PG_HIP(hipMemcpyAsync(rad.data(), ix->d_rad, (size_t)nl * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(off.data(), ix->d_off, ((size_t)nl + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    ix->nonfinite = h_flag != 0;
    ix->st.n_lists = nl;
    ix->st.dim = dim;
    ix->st.rows = rows;
    list_summary(rad, off, &ix->st);
    return PG_OK;
}

// ---- refresh: host --------------------------------------------------------------------------------
constexpr uint32_t kReassignChunk = 1u << 18;        // rows gathered per assign_kernel launch (128 MB at dim 128)

// the rule's list of the rows ids[0, count) (device), computed by assign_kernel over a gathered copy of them and patched into
// assign; xg: [kReassignChunk][dim], vals: [kReassignChunk]
int reassign_rows(pg_ctx* ctx, const pg_table* t, const float* C, float* cn2, uint32_t nl, const uint32_t* ids, uint64_t count, float* xg,
                  uint32_t* vals, uint32_t* assign, uint32_t* flag, unsigned long long* moved) {
    int rc;
    for (uint64_t at = 0; at < count; at += kReassignChunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(kReassignChunk, count - at);
        if ((rc = table_gather_locked(ctx, t, ids + at, m, xg))) return rc;
        if ((rc = assign_dispatch(ctx, t->dim, xg, m, C, cn2, nl, vals, flag))) return rc;
        patch_kernel<<<(m + 255) / 256, 256, 0, ctx->stream>>>(ids + at, vals, m, t->rows, assign, moved);
        PG_HIP(hipGetLastError());
    }
    return PG_OK;
}

struct RefreshOut {                      // what a refresh built (owned until installed) and counted
    uint32_t* perm = nullptr;
    void* small = nullptr;
    bool nonfinite = false;
    uint64_t reassigned = 0, moved = 0, wide = 0;
    double assign_ms = 0.0;
    std::vector<float> rad;
    std::vector<uint32_t> off;
};

// The new permutation, offsets and radii of ix for the table's current rows and ix's centroids, in new buffers; caller holds
// ctx->mu and the table's shared lock.  incremental: only the rows of the table's write log are re-assigned.
int index_refresh_locked(pg_ctx* ctx, const pg_index* ix, bool incremental, RefreshOut* o, std::vector<void*>& owned,
                         std::vector<void*>& temp, hipEvent_t ev0, hipEvent_t ev1) {
    const pg_table* t = ix->t;
    const uint64_t rows = ix->rows;
    const uint32_t dim = ix->dim, nl = ix->n_lists;
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = dalloc((void**)&o->perm, rows * 4, owned))) return rc;
    const size_t off_b = align_up((size_t)(nl + 1) * 4), cent_b = (size_t)nl * dim * 4, lists_b = align_up((size_t)nl * 4);
    if ((rc = dalloc(&o->small, off_b + cent_b + 2 * lists_b, owned))) return rc;
    uint32_t* const n_off = (uint32_t*)o->small;
    float* const n_cent = (float*)((char*)o->small + off_b);
    float* const n_cnorm = (float*)((char*)n_cent + cent_b);
    float* const n_rad = (float*)((char*)n_cnorm + lists_b);
    float *cn2, *xg;
    uint32_t *assign, *keys_s, *vals_in, *vals, *flag;
    if ((rc = dalloc((void**)&cn2, (size_t)nl * 4, temp))) return rc;
    if ((rc = dalloc((void**)&assign, rows * 4, temp))) return rc;
    if ((rc = dalloc((void**)&keys_s, rows * 4, temp))) return rc;
    if ((rc = dalloc((void**)&vals_in, rows * 4, temp))) return rc;
    if ((rc = dalloc((void**)&flag, 32, temp))) return rc;
    const uint64_t chunk = std::min<uint64_t>(kReassignChunk, rows);
    if ((rc = dalloc((void**)&xg, chunk * dim * 4, temp))) return rc;
    if ((rc = dalloc((void**)&vals, chunk * 4, temp))) return rc;
    size_t tmp_bytes = 0;
    void* tmp;
    if ((rc = sort_temp_bytes(rows, nl, &tmp_bytes))) return rc;
    if ((rc = dalloc(&tmp, tmp_bytes, temp))) return rc;
    unsigned long long* const moved = (unsigned long long*)(flag + 2);        // flag[0] non-finite, flag[1] wide rows, [2, 4) moved
    PG_HIP(hipMemsetAsync(flag, 0, 32, s));
    // the centroids and their norms stay: bit copies
    PG_HIP(hipMemcpyAsync(n_cent, ix->d_cent, cent_b, hipMemcpyDeviceToDevice, s));
    PG_HIP(hipMemcpyAsync(n_cnorm, ix->d_cnorm, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
    // the lists the index holds now, per row (the full path counts the moved rows against them)
    uint32_t* const old_assign = incremental ? assign : vals_in;
    list_of_row_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(ix->d_perm, ix->d_off, rows, nl, old_assign);
    PG_HIP(hipGetLastError());
    PG_HIP(hipEventRecord(ev0, s));
    if (incremental) {
        // the log's rows, gathered and re-assigned by the rule's own kernel, patched into the recovered lists
        uint64_t d_rows = 0;
        for (uint32_t i = 0; i < t->log_n; ++i) d_rows += t->log_hi[i] - t->log_lo[i];
        uint32_t* ids = keys_s;              // (free until the sort)
        uint64_t at = 0;
        for (uint32_t i = 0; i < t->log_n; ++i) {
            const uint64_t m = t->log_hi[i] - t->log_lo[i];
            iota_from_kernel<<<(uint32_t)((m + 255) / 256), 256, 0, s>>>(ids + at, m, (uint32_t)t->log_lo[i]);
            PG_HIP(hipGetLastError());
            at += m;
        }
        if ((rc = reassign_rows(ctx, t, ix->d_cent, cn2, nl, ids, d_rows, xg, vals, assign, flag, moved))) return rc;
        o->reassigned = d_rows;
        if (ix->nonfinite) {                 // (which rows were not finite is not recorded: look at all of them)
            PG_HIP(hipMemsetAsync(flag, 0, 4, s));
            finite_kernel<<<(uint32_t)ctx->num_cus * 8, 256, 0, s>>>(t->d, rows * dim, flag);
            PG_HIP(hipGetLastError());
        }
    } else {
        bool screened = false;
        if (dim == 64 || dim == 128) {
            void* ws;
            uint32_t* const wide = keys_s;   // (free until the sort)
            if ((rc = dalloc(&ws, assign_screen_ws_bytes(nl, dim), temp))) return rc;
            rc = assign_screen_launch(ctx, dim, t->d, rows, ix->d_cent, nl, ws, assign, wide, flag + 1, flag);
            if (rc == PG_OK) {
                screened = true;
                uint32_t h_wide = 0;
                PG_HIP(hipMemcpyAsync(&h_wide, flag + 1, 4, hipMemcpyDeviceToHost, s));
                PG_HIP(hipStreamSynchronize(s));
                // the rows the screen left open: the fp32 kernel against all lists (`assign` holds nothing for them yet: the
                // moved rows are counted against old_assign below)
                if ((rc = reassign_rows(ctx, t, ix->d_cent, cn2, nl, wide, h_wide, xg, vals, assign, flag, nullptr))) return rc;
                o->wide = h_wide;
            } else if (rc != PG_ERR_UNSUPPORTED) {
                return rc;
            }
        }
        // (a centroid outside the screen's range, dim 192 / 256: the fp32 kernel for every row)
        if (!screened && (rc = assign_dispatch(ctx, dim, t->d, rows, ix->d_cent, cn2, nl, assign, flag))) return rc;
        count_moved_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(old_assign, assign, rows, moved);
        PG_HIP(hipGetLastError());
        o->reassigned = rows;
    }
    PG_HIP(hipEventRecord(ev1, s));
    // the build's steps: the stable sort by list is the permutation, offsets, radii over the rows actually assigned
    if ((rc = sort_by_list(ctx, assign, rows, nl, keys_s, vals_in, o->perm, n_off, tmp, tmp_bytes))) return rc;
    PG_HIP(hipMemsetAsync(n_rad, 0, (size_t)nl * 4, s));
    radius_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(t->d, rows, dim, assign, ix->d_cent, (uint32_t*)n_rad);
    PG_HIP(hipGetLastError());
    o->rad.resize(nl);
    o->off.resize((size_t)nl + 1);
    uint32_t h_flag[4] = {0, 0, 0, 0};
    PG_HIP(hipMemcpyAsync(o->rad.data(), n_rad, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipMemcpyAsync(o->off.data(), n_off, ((size_t)nl + 1) * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipMemcpyAsync(h_flag, flag, 16, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    o->nonfinite = h_flag[0] != 0;
    memcpy(&o->moved, h_flag + 2, 8);
    float ms = 0.0f;
    PG_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    o->assign_ms = ms;
    return PG_OK;
}

// kSlotIndexSearch of one batch (NOMEM instead of a device error when it cannot grow): U [nq][nl] | qn [nq] f64 | nqv [nq] | Bkey [nq] | probe rows [nq] | counts [nq] | the plan's words [16] |
//          slice counts [nq][kSlices] | scan threshold [nq]
struct SearchBufs {
    float* U;
    double* qn;
    float* nqv;
    uint32_t *Bkey, *probe, *dcount;
    IndexPlanWords* pw;
    uint32_t* cntg;
    float* thr_scan;                     // the probe's K-th scores, frozen for the scan's list selection
};
int search_bufs(pg_ctx* ctx, uint32_t nq, uint32_t nl, SearchBufs* b) {
    const int rc = scratch_carve(ctx, kSlotIndexSearch, [&](Carve& c) {
        b->U = c.take<float>((size_t)nq * nl);
        b->qn = c.take<double>(nq);
        b->nqv = c.take<float>(nq);
        b->Bkey = c.take<uint32_t>(nq);
        b->probe = c.take<uint32_t>(nq);
        b->dcount = c.take<uint32_t>(nq);
        uint32_t* words = c.take<uint32_t>(16 + (size_t)nq * kSlices);      // ONE region: the plan's 16 words, the slice counts behind them
        b->pw = (IndexPlanWords*)words;
        b->cntg = words + 16;
        b->thr_scan = c.take<float>(nq);
    }, true);
    return rc ? PG_ERR_NOMEM : PG_OK;
}

// the bounds of a batch: qn[q] >= ||q|| (and *flag |= 1 for a non-finite query), then U[q][L] — the one launch of the
// search and pg_index_bounds
int bounds_launch(pg_ctx* ctx, const pg_index* ix, const float* d_q, uint32_t nq, bool l2, double* qn, uint32_t* flag, float* U) {
    const uint32_t nl = ix->n_lists, dim = ix->dim;
    hipStream_t s = ctx->stream;
    qinfo_kernel<<<nq, 64, 0, s>>>(d_q, dim, qn, flag);
    const dim3 bg((nl + 255) / 256, (nq + kBoundQ - 1) / kBoundQ);
    const size_t blds = (size_t)kBoundQ * dim * 8;
    if (l2) bound_kernel<true><<<bg, 256, blds, s>>>(d_q, nq, dim, qn, ix->d_cent, ix->d_cnorm, ix->d_rad, nl, U);
    else bound_kernel<false><<<bg, 256, blds, s>>>(d_q, nq, dim, qn, ix->d_cent, ix->d_cnorm, ix->d_rad, nl, U);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// The lists a search walks: the index's own, or a filter's — the same sequence over either.  rows: the rows
// the lists hold (the probe covers min(K, rows) of them); dense_rows: the rows the dense rule weighs the batch's pairs against.
struct SearchLists {
    const uint32_t* perm;
    const uint32_t* off;
    uint64_t rows;
    double dense_rows;
};
SearchLists own_lists(const pg_index* ix) { return SearchLists{ix->d_perm, ix->d_off, ix->rows, (double)ix->rows}; }

// The search of one batch, enqueued on ctx->stream: plan init, the L2 query norms, bounds, probe, the probe's count, plan kernel
// and rounds, the frozen scan threshold, the scan's count and union, plan kernel and rounds, final, the negation for L2.  The
// device writes its verdict into sb.pw and every round's expansion reads it.  Two round policies:
//   h_pw null   an attached plan: `budget` rounds per stage on one grid, no host reads (rounds past the verdict's do nothing)
//   h_pw        the synchronous call (budget unlimited): after each stage's plan kernel the host reads the words into *h_pw; a
//               flag ends the search there (that stage's pairs cleared: not scored), else the stage runs exactly its rounds,
//               each on a grid sized to its suspects
int index_search(pg_ctx* ctx, const pg_index* ix, const SearchLists& li, const float* d_q, uint32_t nq, uint32_t k, bool l2, RecallScratch& rs,
                 const SearchBufs& sb, uint64_t* d_rows, float* d_sc, uint32_t* d_count, uint32_t budget, IndexPlanWords* h_pw) {
    const pg_table* t = ix->t;
    const uint32_t nl = ix->n_lists, dim = t->dim;
    hipStream_t s = ctx->stream;
    int rc;
    index_plan_init_kernel<<<1, kMaxQueries, 0, s>>>(rs.thr, rs.cnt, rs.overflow, sb.pw);
    PG_HIP(hipGetLastError());
    if (l2 && (rc = query_norm2_launch(ctx, d_q, nq, dim, sb.nqv))) return rc;
    if ((rc = bounds_launch(ctx, ix, d_q, nq, l2, sb.qn, &sb.pw->flags, sb.U))) return rc;
    probe_kernel<<<nq, 1024, 0, s>>>(sb.U, nl, li.off, li.rows, k, sb.Bkey, sb.probe);
    count_kernel<<<dim3(kSlices, nq), 256, 0, s>>>(sb.U, nl, li.off, sb.Bkey, rs.thr, 0, sb.cntg);
    PG_HIP(hipGetLastError());
    // the dense rule: the scan gathers a full row per pair, the table's pass streams a shadow whose cost grows slowly with the
    // batch: at 100 M rows the index breaks even at about 0.010 / 0.038 / 0.085 / 0.16 / 0.3-0.5 x rows pairs for 1 / 8 / 32 / 64 /
    // 256 queries (profiles/index_breakeven.json with profiles/index_sweep_10k.json) — 0.01 x rows x nq^0.6 (a
    // filter's lists: dense_rows)
    const double limit = ctx->knobs.index_dense_fraction * li.dense_rows * std::pow((double)nq, 0.6);
    const uint32_t scap = rs.cap - k;
    // a round of n suspects per query: one block per 1024, at most max(16, 4096 / nq) (the blocks past a query's suspects return)
    auto grid = [&](uint64_t n) {
        return std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((n + 1023) / 1024, std::max<uint32_t>(16u, 4096u / nq)));
    };
    int cur = 0;
    // score the stage's lists' rows in rounds of scap per query, keeping each query's best K between rounds
    auto stage = [&](int mode) -> int {
        index_plan_kernel<<<1, kMaxQueries, 0, s>>>(sb.cntg, nq, mode, scap, budget, limit, sb.pw);
        PG_HIP(hipGetLastError());
        uint32_t rounds = budget;
        uint64_t most = 0;
        if (h_pw) {
            PG_HIP(hipMemcpyAsync(h_pw, sb.pw, sizeof *h_pw, hipMemcpyDeviceToHost, s));
            PG_HIP(hipStreamSynchronize(s));
            if (h_pw->flags) {
                h_pw->pairs[mode] = 0;
                return PG_OK;
            }
            rounds = h_pw->need[mode];
            most = mode == 0 ? h_pw->max_probe : h_pw->max_scan;
        }
        for (uint32_t r = 0; r < rounds; ++r) {
            expand_kernel<<<dim3(kSlices, nq), 256, 0, s>>>(sb.U, nl, li.off, li.perm, sb.Bkey, sb.thr_scan, mode, sb.cntg, r, scap,
                                                             rs.susp, rs.susp_cnt, sb.pw);
            PG_HIP(hipGetLastError());
            const uint32_t blocks = grid(h_pw ? std::min<uint64_t>(most - (uint64_t)r * scap, scap) : scap);
            int rc3;
            if ((rc3 = rescore_launch(ctx, dim, l2, t->d, d_q, rs.thr, rs.susp, rs.susp_cnt, scap, rs.cnt, rs.cand[cur], rs.overflow, rs.cap,
                                      nq, (uint32_t)ix->rows /* the gather's bound: the table's rows */, l2 ? t->derived.d_nx : nullptr, l2 ? sb.nqv : nullptr, blocks)))
                return rc3;
            // (a round without suspects selects the kept list again: the same K keys, the same threshold)
            if ((rc3 = launch_select(ctx, nq, rs.cand[cur], rs.cand[cur ^ 1], rs.cnt, rs.thr, rs.cap, k, 0))) return rc3;
            cur ^= 1;
        }
        return PG_OK;
    };
    if ((rc = stage(0)) || (h_pw && h_pw->flags)) return rc;
    // the scan: lists outside the probe whose bound reaches the probe's K-th score.  The selection is made ONCE against that
    // threshold (thr_scan): the per-slice counts and every round's expansion must see the same lists, while rs.thr keeps
    // rising with the select between rounds and serves only the re-scoring's candidate test.
    PG_HIP(hipMemcpyAsync(sb.thr_scan, rs.thr, (size_t)nq * 4, hipMemcpyDeviceToDevice, s));
    count_kernel<<<dim3(kSlices, nq), 256, 0, s>>>(sb.U, nl, li.off, sb.Bkey, sb.thr_scan, 1, sb.cntg);
    union_kernel<<<(nl + 255) / 256, 256, 0, s>>>(sb.U, nl, nq, li.off, sb.Bkey, sb.thr_scan, &sb.pw->union_rows);
    PG_HIP(hipGetLastError());
    if ((rc = stage(1)) || (h_pw && h_pw->flags)) return rc;
    if ((rc = final_launch(ctx, rs.cand[cur], rs.cnt, rs.cap, nq, k, t->row_offset, d_rows, d_sc, d_count))) return rc;
    if (l2 && (rc = negate_launch(ctx, d_sc, (uint64_t)nq * k))) return rc;
    return PG_OK;
}

int table_pass_locked(pg_ctx* ctx, const pg_table* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc,
                      uint32_t* h_counts, bool l2) {
    RecallOpts o;
    o.l2 = l2;
    o.no_index = true;                   // (never through an attached index: this is the index's own fallback)
    return recall_batches_locked(ctx, t, d_q, nq, k, d_rows, d_sc, h_counts, o);
}

// one batch, synchronously (caller holds ctx->mu and the table's shared lock); h_counts: host [nq].  A stale, non-finite, dense
// or overflowing batch is answered by the table's pass.
int index_recall_locked(pg_ctx* ctx, pg_index* ix, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc,
                        uint32_t* h_counts, bool l2) {
    const pg_table* t = ix->t;
    const uint32_t dim = t->dim;
    IndexPlanWords w{};                  // the plan words as the host read them last (the pairs of the stages scored)
    uint64_t pg_index_stats_t::*fb = nullptr;          // the fallback the batch takes
    int rc = PG_OK;
    if (t->generation.load(std::memory_order_relaxed) != ix->gen) fb = &pg_index_stats_t::fallback_stale;
    else if (ix->nonfinite) fb = &pg_index_stats_t::fallback_nonfinite;
    else if (l2 && dim != 64 && dim != 128) fb = &pg_index_stats_t::fallback_dense;   // (the table's pass answers with its own error)
    else rc = [&]() -> int {
        RecallScratch rs;
        SearchBufs sb;
        int rc2;
        if ((rc2 = recall_scratch(ctx, dim, k, &rs))) return rc2;
        if (l2 && (rc2 = ensure_table_nx(ctx, t))) return rc2;
        if (search_bufs(ctx, nq, ix->n_lists, &sb)) {
            fb = &pg_index_stats_t::fallback_overflow;
            return PG_OK;
        }
        if ((rc2 = index_search(ctx, ix, own_lists(ix), d_q, nq, k, l2, rs, sb, d_rows, d_sc, sb.dcount, ~0u, &w))) return rc2;
        if (w.flags & kPlanNonfinite) fb = &pg_index_stats_t::fallback_nonfinite;
        else if (w.flags & kPlanDense) fb = &pg_index_stats_t::fallback_dense;
        if (fb) return PG_OK;
        uint32_t h_ovf = 0;
        PG_HIP(hipMemcpyAsync(&h_ovf, rs.overflow, 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipMemcpyAsync(h_counts, sb.dcount, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        if (h_ovf) fb = &pg_index_stats_t::fallback_overflow;
        return PG_OK;
    }();
    if (rc == PG_OK && fb) rc = table_pass_locked(ctx, t, d_q, nq, k, d_rows, d_sc, h_counts, l2);
    if (rc != PG_OK) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->st.calls++;
    ix->st.queries += nq;
    ix->st.pairs_scored += w.pairs[0] + w.pairs[1];
    ix->st.rows_scored += w.pairs[0] + w.pairs[1];
    ix->st.rows_live += w.union_rows;
    ix->st.max_query_scan_rows = std::max<uint64_t>(ix->st.max_query_scan_rows, w.max_scan);
    if (fb) ix->st.*fb += 1;
    return PG_OK;
}

// pg_index_recall_topk[_l2][_dev]: host, the queries and outputs are host memory (staged through kSlotStaging)
int index_entry(const char* who, pg_ctx* ctx, const pg_index* ixc, const float* q, uint32_t nq, uint32_t k, uint64_t* rows, float* sc,
                uint32_t* out_count, bool l2, bool host) {
    int rc;
    if ((rc = recall_check(who, ctx, ixc, q, rows, sc, nq, k, l2))) return rc;
    pg_index* ix = const_cast<pg_index*>(ixc);          // (only the statistics change)
    std::lock_guard<std::mutex> g(ctx->mu);
    TableRead tr(ix->t->rw);
    uint32_t counts[kMaxQueries];
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return index_recall_locked(ctx, ix, d_q, nq, k, d_rows, d_sc, counts, l2);
    };
    if ((rc = host ? recall_staged(ctx, ix->dim, q, nq, k, rows, sc, run) : run(q, rows, sc))) return rc;
    if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
    return PG_OK;
}

int band_of(uint32_t nq) { return nq <= 1 ? 0 : nq <= 8 ? 1 : nq <= 32 ? 2 : nq <= 64 ? 3 : 4; }

// A filter's lists over the index, built on ctx->stream: the predicate's bitmap in row order, the admitted rows per list, their
// exclusive scan (the offsets), then the stable compaction of the permutation.  Synchronises (the total sizes the allocation).
int where_lists_build(pg_ctx* ctx, const pg_index* ix, const RowFilter& f, std::shared_ptr<WhereLists>* out) {
    const uint32_t nl = ix->n_lists;
    const uint64_t rows = ix->rows;
    hipStream_t s = ctx->stream;
    std::vector<void*> temp;
    auto done = [&](int rc) {
        (void)hipStreamSynchronize(s);
        free_all(temp);
        return rc;
    };
    int rc;
    uint32_t *bits = nullptr, *cnt, *off;
    const size_t words = (size_t)((rows + 31) / 32);
    const bool have_bits = f.dtype == kFilterBits;       // (a compound clause's filter IS the bitmap in row order)
    if ((!have_bits && (rc = dalloc((void**)&bits, words * 4, temp))) || (rc = dalloc((void**)&cnt, ((size_t)nl + 1) * 4, temp)) ||
        (rc = dalloc((void**)&off, ((size_t)nl + 1) * 4, temp)))
        return done(rc);
    size_t scan_b = 0;
    void* scan_tmp;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, cnt, off, nl + 1, s) != hipSuccess) return done(PG_ERR_DEVICE);
    if ((rc = dalloc(&scan_tmp, scan_b, temp))) return done(rc);
    if (have_bits) bits = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(f.col));
    else where_bits_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(f, rows, bits);
    if (hipMemsetAsync(cnt + nl, 0, 4, s) != hipSuccess) return done(PG_ERR_DEVICE);
    where_lists_kernel<true><<<nl, 256, 0, s>>>(ix->d_perm, ix->d_off, bits, cnt, nullptr);
    if (hipGetLastError() != hipSuccess || hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_b, cnt, off, nl + 1, s) != hipSuccess)
        return done(PG_ERR_DEVICE);
    uint32_t admitted = 0;
    if (hipMemcpyAsync(&admitted, off + nl, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(PG_ERR_DEVICE);
    auto wl = std::make_shared<WhereLists>();
    const size_t off_b = align_up(((size_t)nl + 1) * 4);
    if (hipMalloc(&wl->d, off_b + (size_t)admitted * 4 + 16) != hipSuccess) {
        (void)hipGetLastError();
        wl->d = nullptr;
        return done(PG_ERR_NOMEM);
    }
    wl->off = (uint32_t*)wl->d;
    wl->perm = (uint32_t*)((char*)wl->d + off_b);
    wl->admitted = admitted;
    wl->bytes = (size_t)admitted * 4 + ((size_t)nl + 1) * 4;
    if (hipMemcpyAsync(wl->off, off, ((size_t)nl + 1) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return done(PG_ERR_DEVICE);
    where_lists_kernel<false><<<nl, 256, 0, s>>>(ix->d_perm, ix->d_off, bits, wl->off, wl->perm);
    if (hipGetLastError() != hipSuccess) return done(PG_ERR_DEVICE);
    rc = done(PG_OK);
    if (rc == PG_OK) *out = std::move(wl);
    return rc;
}

// the filter's lists from the index's cache, or built (and kept while "index_where_cache" of the calling context allows); caller
// holds ctx->mu and the table's shared lock
int where_lists_get(pg_ctx* ctx, pg_index* ix, const WhereId& id, const RowFilter& f, std::shared_ptr<WhereLists>* out) {
    const WhereKey key = id.w ? WhereKey{id.fs, -1, 0, 0, 0, ix->gen, id.w, id.epoch}
                              : WhereKey{id.fs, id.column, id.fs->cols[(size_t)id.column].version, f.op, f.val, ix->gen, nullptr, 0};
    std::lock_guard<std::mutex> g(ix->where_mu);
    pg_index_where_stats_t& st = ix->where_st;
    const uint32_t cap = ctx->knobs.index_where_cache;
    auto trim = [&]() {                      // (to the calling context's capacity: at 0 every call builds)
        while (ix->where_cache.size() > cap) {
            st.evictions++;
            st.bytes -= ix->where_cache.back()->bytes;
            ix->where_cache.pop_back();      // (a search that still holds the entry keeps it alive)
        }
        st.entries = ix->where_cache.size();
    };
    trim();
    for (auto it = ix->where_cache.begin(); it != ix->where_cache.end(); ++it) {
        if (!((*it)->key == key)) continue;
        ix->where_cache.splice(ix->where_cache.begin(), ix->where_cache, it);
        st.hits++;
        *out = ix->where_cache.front();
        return PG_OK;
    }
    int rc;
    if ((rc = where_lists_build(ctx, ix, f, out))) {
        if (rc == PG_ERR_DEVICE) set_error("index filtered lists: %s", hipGetErrorString(hipGetLastError()));
        else set_error("index filtered lists: device allocation failed (%llu rows)", (unsigned long long)ix->rows);
        return rc;
    }
    (*out)->key = key;
    st.builds++;
    if (cap) {
        ix->where_cache.push_front(*out);
        st.bytes += (*out)->bytes;
    }
    trim();
    return PG_OK;
}

}  // namespace

const pg_table* index_table(const pg_index* ix) { return ix->t; }

pg_index* index_route_where(const pg_ctx* ctx, const pg_table* t) {
    if (!ctx->knobs.index_route_where || t->d_row_map) return nullptr;
    pg_index* ix = t->index.load(std::memory_order_acquire);
    return ix && t->generation.load(std::memory_order_relaxed) == ix->gen ? ix : nullptr;
}

// one filtered batch, synchronously (caller holds ctx->mu and the table's shared lock); h_counts: host [nq].  The search of
// index_recall_locked over the filter's lists; a stale, non-finite, dense or overflowing batch is answered by the filtered pass.
int index_where_locked(pg_ctx* ctx, pg_index* ix, const WhereId& id, const RowFilter& f, bool l2, const float* d_q,
                       uint32_t nq, uint32_t k, uint64_t* d_rows, float* d_sc, uint32_t* h_counts) {
    const pg_table* t = ix->t;
    const uint32_t dim = t->dim;
    IndexPlanWords w{};
    uint64_t pg_index_stats_t::*fb = nullptr;
    std::shared_ptr<WhereLists> wl;      // (released after the stream has synchronised: every path below ends synchronised)
    int rc = PG_OK;
    if (t->generation.load(std::memory_order_relaxed) != ix->gen) fb = &pg_index_stats_t::fallback_stale;
    else if (ix->nonfinite) fb = &pg_index_stats_t::fallback_nonfinite;
    else if (l2 && dim != 64 && dim != 128) fb = &pg_index_stats_t::fallback_dense;   // (the filtered pass answers with its own error)
    else rc = [&]() -> int {
        int rc2;
        if ((rc2 = where_lists_get(ctx, ix, id, f, &wl))) return rc2;
        if (wl->admitted == 0) {
            // nothing passes: padding, every count 0 (as pg_recall_topk_where)
            if ((rc2 = where_pad_launch(ctx, d_rows, d_sc, (size_t)nq * k, l2))) return rc2;
            for (uint32_t q = 0; q < nq; ++q) h_counts[q] = 0;
            PG_HIP(hipStreamSynchronize(ctx->stream));
            return PG_OK;
        }
        RecallScratch rs;
        SearchBufs sb;
        if ((rc2 = recall_scratch(ctx, dim, k, &rs))) return rc2;
        if (l2 && (rc2 = ensure_table_nx(ctx, t))) return rc2;
        if (search_bufs(ctx, nq, ix->n_lists, &sb)) {
            fb = &pg_index_stats_t::fallback_overflow;
            return PG_OK;
        }
        // the dense rule weighs the pairs against the filtered pass, which streams the table or gathers a compact copy of the
        // admitted rows, whichever is less
        const SearchLists li{wl->perm, wl->off, wl->admitted, std::min((double)ix->rows, kWhereGatherWeight * (double)wl->admitted)};
        if ((rc2 = index_search(ctx, ix, li, d_q, nq, k, l2, rs, sb, d_rows, d_sc, sb.dcount, ~0u, &w))) return rc2;
        if (w.flags & kPlanNonfinite) fb = &pg_index_stats_t::fallback_nonfinite;
        else if (w.flags & kPlanDense) fb = &pg_index_stats_t::fallback_dense;
        if (fb) return PG_OK;
        uint32_t h_ovf = 0;
        PG_HIP(hipMemcpyAsync(&h_ovf, rs.overflow, 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipMemcpyAsync(h_counts, sb.dcount, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        if (h_ovf) fb = &pg_index_stats_t::fallback_overflow;
        return PG_OK;
    }();
    if (rc != PG_OK && wl) (void)hipStreamSynchronize(ctx->stream);
    wl.reset();
    if (rc == PG_OK && fb) rc = recall_where_locked(ctx, t, f, l2 ? 1 : 0, d_q, nq, k, d_rows, d_sc, h_counts);
    if (rc != PG_OK) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->st.calls++;
    ix->st.queries += nq;
    ix->st.pairs_scored += w.pairs[0] + w.pairs[1];
    ix->st.rows_scored += w.pairs[0] + w.pairs[1];
    ix->st.rows_live += w.union_rows;
    ix->st.max_query_scan_rows = std::max<uint64_t>(ix->st.max_query_scan_rows, w.max_scan);
    if (fb) ix->st.*fb += 1;
    return PG_OK;
}

// ---- an attached index as a RecallJob plan ------------------------------------------------------------------------
// In front of the table's plans when the table has an attachment that is current and finite, and the job is one the index
// serves (no filter, not exact_only, not a view, not the index's own fallback or the shard group); the batch's size band may
// be switched off for a while (index_plan_check).  Caller holds ctx->mu and the table's shared lock.
int index_plan_prepare(RecallJob* j) {
    const pg_table* t = j->t;
    j->ix = nullptr;
    j->ix_serve.reset();
    pg_index* ix = t->index.load(std::memory_order_acquire);
    if (!ix || j->no_index || j->filter.col || j->exact_only || j->skip_pilot || t->d_row_map) return PG_OK;
    IndexServe& sv = *ix->serve;
    if (t->generation.load(std::memory_order_relaxed) != ix->gen) {
        sv.skipped_stale++;
        return PG_OK;
    }
    if (ix->nonfinite || j->k > 16384 || (j->l2 && t->dim != 64 && t->dim != 128) || (!j->l2 && t->dim > 128 && j->nq > 32)) return PG_OK;
    std::atomic<int32_t>& sw = sv.skip[band_of(j->nq)];
    int32_t left = sw.load(std::memory_order_relaxed);
    while (left > 0 && !sw.compare_exchange_weak(left, left - 1, std::memory_order_relaxed)) {}
    if (left > 0) {
        sv.skipped_switch++;
        return PG_OK;
    }
    SearchBufs room;
    if (search_bufs(j->ctx, j->nq, ix->n_lists, &room)) return PG_OK;     // (no memory: the table's plans)
    for (int i = j->n_plans; i > 0; --i) j->plans[i] = j->plans[i - 1];
    j->plans[0] = kIndexPlan;
    j->n_plans++;
    j->next_plan = 0;
    j->ix = ix;
    j->ix_serve = ix->serve;
    return PG_OK;
}

// index_search with the attached plan's round policy (index_plan_rounds per stage, no host reads) between the job's events; the
// outputs, the status block and its copy as any plan's
int index_plan_enqueue(RecallJob* j, uint32_t status_words) {
    pg_ctx* ctx = j->ctx;
    const uint32_t nq = j->nq;
    RecallScratch& rs = j->rs;
    hipStream_t s = ctx->stream;
    int rc;
    SearchBufs sb;
    if ((rc = search_bufs(ctx, nq, j->ix->n_lists, &sb))) return rc;      // (reserved by index_plan_prepare: only grows)
    while (j->events->size() < 2) {
        hipEvent_t e;
        PG_HIP(hipEventCreate(&e));
        j->events->push_back(e);
    }
    j->timers = !ctx->timers_off;
    if (j->timers) PG_HIP(hipEventRecord((*j->events)[0], s));
    const uint32_t budget = ctx->knobs.index_plan_rounds ? ctx->knobs.index_plan_rounds : 1u;
    if ((rc = index_search(ctx, j->ix, own_lists(j->ix), j->d_queries, nq, j->k, j->l2, rs, sb, j->d_out_rows, j->d_out_scores, j->d_count, budget, nullptr)))
        return rc;
    if (j->timers) PG_HIP(hipEventRecord((*j->events)[1], s));
    index_status_kernel<<<1, kMaxQueries, 0, s>>>(rs.overflow, nq, sb.pw, rs.status);
    PG_HIP(hipGetLastError());
    if (j->d_out_count) PG_HIP(hipMemcpyAsync(j->d_out_count, j->d_count, 4 * (size_t)nq, hipMemcpyDeviceToDevice, s));
    PG_HIP(hipMemcpyAsync(j->h_status, rs.status, 4 * (size_t)status_words, hipMemcpyDeviceToHost, s));
    j->n_ev = 1;
    j->refined = j->observed = j->susp_stat = j->stat_wide = false;
    j->enqueued_plan = kIndexPlan;
    j->next_plan++;
    return PG_OK;
}

// the verdict of an enqueued index plan (its status words have arrived): held, or a reason to let the table's first plan serve
// the whole batch — dense and rounds also switch the batch's size band off for index_skip_batches batches
int index_plan_check(RecallJob* j, bool* ok) {
    IndexServe& sv = *j->ix_serve;
    IndexPlanWords w;
    memcpy(&w, j->h_status + kIndexStatAt, sizeof w);
    sv.plans++;
    sv.queries += j->nq;
    j->failed.clear();
    *ok = false;
    if (w.flags & kPlanNonfinite) {
        sv.replan_nonfinite++;
    } else if (w.flags & (kPlanDense | kPlanRounds)) {
        if (w.flags & kPlanDense) sv.replan_dense++;
        else sv.replan_rounds++;
        sv.skip[band_of(j->nq)].store((int32_t)std::min<uint32_t>(j->ctx->knobs.index_skip_batches, 0x7FFFFFFFu), std::memory_order_relaxed);
    } else if (j->h_status[0] != 0) {
        sv.replan_overflow++;
    } else {
        *ok = true;
        sv.plans_held++;
        sv.queries_held += j->nq;
        sv.pairs += w.pairs[0] + w.pairs[1];
        sv.rows_live += w.union_rows;
        uint64_t m = sv.max_scan.load(std::memory_order_relaxed);
        while (w.max_scan > m && !sv.max_scan.compare_exchange_weak(m, w.max_scan, std::memory_order_relaxed)) {}
    }
    if (j->ctx->knobs.debug_scan)
        fprintf(stderr, "[pg] index plan %s: flags %u, rounds %u + %u, pairs %llu + %llu\n", *ok ? "held" : "re-planned", w.flags, w.need[0],
                w.need[1], w.pairs[0], w.pairs[1]);
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_index_build(pg_ctx* ctx, const pg_table* t, const pg_index_params* p, pg_index** out) {
    PG_REQUIRE(ctx && t && out, "pg_index_build: NULL argument");
    if (t->d_row_map) {
        pg::set_error("pg_index_build: a view cannot be indexed (build the index over the source table)");
        return PG_ERR_UNSUPPORTED;
    }
    if (t->rows >= (1ull << 32)) {
        pg::set_error("pg_index_build: %llu rows unsupported (row ids are 32-bit)", (unsigned long long)t->rows);
        return PG_ERR_UNSUPPORTED;
    }
    const pg_index_params params = p ? *p : pg_index_params{0, 0, 0, 0};
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    const auto t0 = std::chrono::steady_clock::now();
    pg_index* ix = new pg_index();
    ix->t = t;
    ix->gen = t->generation.load(std::memory_order_relaxed);
    ix->rows = t->rows;
    ix->dim = t->dim;
    std::vector<void*> owned, temp;
    int rc = pg::index_build_locked(ctx, t, params, ix, owned, temp);
    if (rc == PG_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        pg::set_error("pg_index_build: %s", hipGetErrorString(hipGetLastError()));
        rc = PG_ERR_DEVICE;
    }
    if (rc != PG_OK) (void)hipStreamSynchronize(ctx->stream);
    pg::free_all(temp);
    if (rc != PG_OK) {
        if (rc == PG_ERR_NOMEM) pg::set_error("pg_index_build: device allocation failed (%llu rows x %u)", (unsigned long long)t->rows, t->dim);
        pg::free_all(owned);
        delete ix;
        return rc;
    }
    ix->st.generation = ix->gen;
    ix->st.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = ix;
    return PG_OK;
}

int pg_index_refresh(pg_ctx* ctx, pg_index* ix, const pg_index_refresh_params* p) {
    PG_REQUIRE(ctx && ix, "pg_index_refresh: NULL argument");
    const pg_index_refresh_params prm = p ? *p : pg_index_refresh_params{0, 0};
    PG_REQUIRE(prm.mode >= 0 && prm.mode <= 2, "pg_index_refresh: mode %d unknown (0 auto, 1 full, 2 incremental)", prm.mode);
    const pg_table* t = ix->t;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::lock_guard<std::mutex> gr(ix->refresh_mu);
    const auto t0 = std::chrono::steady_clock::now();
    pg::TableRead tr(t->rw);
    const uint64_t gen = t->generation.load(std::memory_order_relaxed);
    if (gen == ix->gen && !prm.force) {
        std::lock_guard<std::mutex> gs(ix->mu);
        ix->rst.refreshes++;
        ix->rst.noop++;
        return PG_OK;
    }
    // the write log covers every write since the index's generation?
    const bool covered = ix->gen >= t->log_since;
    uint64_t logged = 0;
    for (uint32_t i = 0; i < t->log_n; ++i) logged += t->log_hi[i] - t->log_lo[i];
    bool incremental;
    if (prm.mode == 2) {
        if (!covered) {
            pg::set_error("pg_index_refresh: the table's write log starts at generation %llu, the index describes %llu (refresh in full)",
                          (unsigned long long)t->log_since, (unsigned long long)ix->gen);
            return PG_ERR_UNSUPPORTED;
        }
        incremental = true;
    } else if (prm.mode == 1 || gen == ix->gen) {
        incremental = false;
    } else {
        incremental = covered && (double)logged <= ctx->knobs.index_refresh_full_fraction * (double)ix->rows;
    }
    PG_HIP(hipSetDevice(ctx->device));
    hipEvent_t ev[2] = {nullptr, nullptr};
    PG_HIP(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) {
        (void)hipEventDestroy(ev[0]);
        pg::set_error("pg_index_refresh: %s", hipGetErrorString(hipGetLastError()));
        return PG_ERR_DEVICE;
    }
    pg::RefreshOut o;
    std::vector<void*> owned, temp;
    int rc = pg::index_refresh_locked(ctx, ix, incremental, &o, owned, temp, ev[0], ev[1]);
    if (rc != PG_OK) (void)hipStreamSynchronize(ctx->stream);
    pg::free_all(temp);
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    if (rc != PG_OK) {
        if (rc == PG_ERR_NOMEM) pg::set_error("pg_index_refresh: device allocation failed (%llu rows x %u)", (unsigned long long)ix->rows, ix->dim);
        pg::free_all(owned);
        return rc;                           // (the index as it was: stale and valid)
    }
    // install as pg_index_attach replaces an index: the table exclusively (no generation bump), the device drained so that no
    // enqueued index plan reads the old arrays, then the exchange.  A write between the two locks leaves the index stale again.
    tr.unlock();
    uint32_t* const old_perm = ix->d_perm;
    void* const old_small = ix->d_small;
    {
        std::unique_lock<std::shared_mutex> w(t->rw);
        if (hipDeviceSynchronize() != hipSuccess) {
            pg::set_error("pg_index_refresh: %s", hipGetErrorString(hipGetLastError()));
            pg::free_all(owned);
            return PG_ERR_DEVICE;
        }
        const uint32_t nl = ix->n_lists;
        const size_t off_b = pg::align_up((size_t)(nl + 1) * 4), cent_b = (size_t)nl * ix->dim * 4, lists_b = pg::align_up((size_t)nl * 4);
        ix->d_perm = o.perm;
        ix->d_small = o.small;
        ix->d_off = (uint32_t*)ix->d_small;
        ix->d_cent = (float*)((char*)ix->d_small + off_b);
        ix->d_cnorm = (float*)((char*)ix->d_cent + cent_b);
        ix->d_rad = (float*)((char*)ix->d_cnorm + lists_b);
        ix->gen = gen;
        ix->nonfinite = o.nonfinite;
        {
            std::lock_guard<std::mutex> gw(ix->where_mu);       // (the cached filters' keys carry the old generation)
            ix->where_cache.clear();
            ix->where_st.entries = 0;
            ix->where_st.bytes = 0;
        }
        std::lock_guard<std::mutex> gs(ix->mu);
        ix->st.generation = gen;
        pg::list_summary(o.rad, o.off, &ix->st);
        pg_index_refresh_stats_t& r = ix->rst;
        r.refreshes++;
        (incremental ? r.incremental : r.full)++;
        r.rows_reassigned += o.reassigned;
        r.rows_moved += o.moved;
        r.rows_confirmed_wide += o.wide;
        r.last_generation = gen;
        r.last_assign_ms = o.assign_ms;
        r.last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    (void)hipFree(old_perm);
    (void)hipFree(old_small);
    return PG_OK;
}

int pg_index_refresh_stats(const pg_index* ixc, pg_index_refresh_stats_t* out) {
    PG_REQUIRE(ixc && out, "pg_index_refresh_stats: NULL argument");
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ix->mu);
    *out = ix->rst;
    return PG_OK;
}

int pg_index_destroy(pg_ctx* ctx, pg_index* ix) {
    PG_REQUIRE(ctx, "pg_index_destroy: ctx is NULL");
    if (!ix) return PG_OK;
    PG_REQUIRE(ix->t->index.load(std::memory_order_acquire) != ix, "pg_index_destroy: the index is attached to its table (pg_index_detach first)");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipStreamSynchronize(ctx->stream));
    if (ix->d_perm) PG_HIP(hipFree(ix->d_perm));
    if (ix->d_small) PG_HIP(hipFree(ix->d_small));
    delete ix;
    return PG_OK;
}

int pg_index_recall_topk(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                         float* out_scores, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk", ctx, ix, queries, nq, k, out_rows, out_scores, out_count, false, true);
}

int pg_index_recall_topk_dev(pg_ctx* ctx, const pg_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                             float* d_out_scores, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk_dev", ctx, ix, d_queries, nq, k, d_out_rows, d_out_scores, out_count, false, false);
}

int pg_index_recall_topk_l2(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                            float* out_dist, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk_l2", ctx, ix, queries, nq, k, out_rows, out_dist, out_count, true, true);
}

int pg_index_recall_topk_l2_dev(pg_ctx* ctx, const pg_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                                float* d_out_dist, uint32_t* out_count) {
    return pg::index_entry("pg_index_recall_topk_l2_dev", ctx, ix, d_queries, nq, k, d_out_rows, d_out_dist, out_count, true, false);
}

// the filtered recall through the index: pg_recall_topk_where's checks and contract, over ix's table
int pg_index_recall_topk_where(pg_ctx* ctx, const pg_index* ixc, const pg_features* fs, int column, int op, long long value, int metric,
                               const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(ixc, "pg_index_recall_topk_where: NULL argument");
    pg::RowFilter f;
    int rc;
    if ((rc = pg::where_check("pg_index_recall_topk_where", ctx, ixc->t, fs, column, op, value, metric, queries, out_rows, out_scores, nq, k,
                              &f)))
        return rc;
    pg_index* ix = const_cast<pg_index*>(ixc);          // (only the statistics and the filtered lists' cache change)
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);
    uint32_t counts[pg::kMaxQueries];
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return pg::index_where_locked(ctx, ix, pg::WhereId{fs, column, nullptr, 0}, f, metric == 1, d_q, nq, k, d_rows, d_sc, counts);
    };
    if ((rc = pg::recall_staged(ctx, ix->dim, queries, nq, k, out_rows, out_scores, run))) return rc;
    if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
    return PG_OK;
}

int pg_index_where_read(pg_ctx* ctx, const pg_index* ixc, const pg_features* fs, int column, int op, long long value, uint32_t* offsets,
                        uint32_t* perm, uint64_t* admitted) {
    PG_REQUIRE(ctx && ixc && fs, "pg_index_where_read: NULL argument");
    PG_REQUIRE(column >= 0 && (size_t)column < fs->cols.size(), "pg_index_where_read: column %d out of range", column);
    PG_REQUIRE(op >= 0 && op <= 5, "pg_index_where_read: op %d unknown (0 >, 1 >=, 2 <, 3 <=, 4 ==, 5 !=)", op);
    PG_REQUIRE(fs->rows >= ixc->rows, "pg_index_where_read: the feature store holds %llu rows, the index %llu", (unsigned long long)fs->rows,
               (unsigned long long)ixc->rows);
    const pg_features::Column& c = fs->cols[(size_t)column];
    if ((c.dtype != PG_F_I32 && c.dtype != PG_F_I64) || !c.d) {
        pg::set_error("pg_index_where_read: column \"%s\" must be an int32 / int64 column with values", c.name.c_str());
        return PG_ERR_UNSUPPORTED;
    }
    pg::RowFilter f;
    f.col = c.d;
    f.dtype = c.dtype;
    f.op = op;
    f.val = value;
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);
    std::shared_ptr<pg::WhereLists> wl;
    int rc;
    if ((rc = pg::where_lists_get(ctx, ix, pg::WhereId{fs, column, nullptr, 0}, f, &wl))) return rc;
    hipStream_t s = ctx->stream;
    if (offsets) PG_HIP(hipMemcpyAsync(offsets, wl->off, ((size_t)ix->n_lists + 1) * 4, hipMemcpyDeviceToHost, s));
    if (perm && wl->admitted) PG_HIP(hipMemcpyAsync(perm, wl->perm, (size_t)wl->admitted * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    if (admitted) *admitted = wl->admitted;
    return PG_OK;
}

int pg_index_where_stats(const pg_index* ixc, pg_index_where_stats_t* out) {
    PG_REQUIRE(ixc && out, "pg_index_where_stats: NULL argument");
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ix->where_mu);
    *out = ix->where_st;
    return PG_OK;
}

int pg_index_stats(const pg_index* ixc, pg_index_stats_t* out) {
    PG_REQUIRE(ixc && out, "pg_index_stats: NULL argument");
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ix->mu);
    *out = ix->st;
    // (+ the batches that tried the attached plan; `rounds` re-plans have no field of their own here)
    const pg::IndexServe& sv = *ix->serve;
    const uint64_t pairs = sv.pairs.load();
    out->calls += sv.plans.load();
    out->queries += sv.queries.load();
    out->rows_scored += pairs;
    out->pairs_scored += pairs;
    out->rows_live += sv.rows_live.load();
    out->max_query_scan_rows = std::max<uint64_t>(out->max_query_scan_rows, sv.max_scan.load());
    out->fallback_dense += sv.replan_dense.load();
    out->fallback_nonfinite += sv.replan_nonfinite.load();
    out->fallback_overflow += sv.replan_overflow.load();
    return PG_OK;
}

int pg_index_read(pg_ctx* ctx, const pg_index* ix, uint32_t* offsets, uint32_t* perm, float* centroids, float* cnorm, float* radius) {
    PG_REQUIRE(ctx && ix, "pg_index_read: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);             // (pg_index_refresh exchanges the arrays under the exclusive lock)
    hipStream_t s = ctx->stream;
    const size_t nl = ix->n_lists;
    if (offsets) PG_HIP(hipMemcpyAsync(offsets, ix->d_off, (nl + 1) * 4, hipMemcpyDeviceToHost, s));
    if (perm) PG_HIP(hipMemcpyAsync(perm, ix->d_perm, (size_t)ix->rows * 4, hipMemcpyDeviceToHost, s));
    if (centroids) PG_HIP(hipMemcpyAsync(centroids, ix->d_cent, nl * ix->dim * 4, hipMemcpyDeviceToHost, s));
    if (cnorm) PG_HIP(hipMemcpyAsync(cnorm, ix->d_cnorm, nl * 4, hipMemcpyDeviceToHost, s));
    if (radius) PG_HIP(hipMemcpyAsync(radius, ix->d_rad, nl * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    return PG_OK;
}

int pg_index_bounds(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, int l2, float* out) {
    PG_REQUIRE(ctx && ix && queries && out, "pg_index_bounds: NULL argument");
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)pg::kMaxQueries, "pg_index_bounds: nq=%u must be in [1,%d]", nq, pg::kMaxQueries);
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);
    hipStream_t s = ctx->stream;
    const size_t qb = (size_t)nq * ix->dim * 4;
    void* buf;
    int rc;
    if ((rc = pg::scratch_reserve(ctx, pg::kSlotStaging, qb, &buf))) return rc;
    pg::SearchBufs sb;
    if ((rc = pg::search_bufs(ctx, nq, ix->n_lists, &sb))) return rc;
    PG_HIP(hipMemcpyAsync(buf, queries, qb, hipMemcpyHostToDevice, s));
    PG_HIP(hipMemsetAsync(&sb.pw->flags, 0, 4, s));
    if ((rc = pg::bounds_launch(ctx, ix, (const float*)buf, nq, l2 != 0, sb.qn, &sb.pw->flags, sb.U))) return rc;
    PG_HIP(hipMemcpyAsync(out, sb.U, (size_t)nq * ix->n_lists * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    return PG_OK;
}

// Attach / detach change no rows: the table's lock is taken exclusively WITHOUT a generation bump (TableWrite's), and the
// device is drained so that nothing enqueued still reads a previous attachment's arrays.
int pg_index_attach(pg_ctx* ctx, pg_index* ix) {
    PG_REQUIRE(ctx && ix, "pg_index_attach: NULL argument");
    PG_REQUIRE(!ix->t->d_row_map, "pg_index_attach: the table is a view");
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> w(ix->t->rw);
    pg_index* prev = ix->t->index.load(std::memory_order_acquire);
    if (prev == ix) return PG_OK;
    if (prev) {
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipDeviceSynchronize());
    }
    ix->t->index.store(ix, std::memory_order_release);
    return PG_OK;
}

int pg_index_detach(pg_ctx* ctx, pg_index* ix) {
    PG_REQUIRE(ctx && ix, "pg_index_detach: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    std::unique_lock<std::shared_mutex> w(ix->t->rw);
    PG_REQUIRE(ix->t->index.load(std::memory_order_acquire) == ix, "pg_index_detach: the index is not attached");
    PG_HIP(hipSetDevice(ctx->device));
    PG_HIP(hipDeviceSynchronize());
    ix->t->index.store(nullptr, std::memory_order_release);
    return PG_OK;
}

int pg_index_serving_stats(const pg_index* ix, pg_index_serving_stats_t* out) {
    PG_REQUIRE(ix && out, "pg_index_serving_stats: NULL argument");
    const pg::IndexServe& sv = *ix->serve;
    out->plans = sv.plans.load();
    out->plans_held = sv.plans_held.load();
    out->queries_held = sv.queries_held.load();
    out->replan_dense = sv.replan_dense.load();
    out->replan_rounds = sv.replan_rounds.load();
    out->replan_overflow = sv.replan_overflow.load();
    out->replan_nonfinite = sv.replan_nonfinite.load();
    out->skipped_stale = sv.skipped_stale.load();
    out->skipped_switch = sv.skipped_switch.load();
    return PG_OK;
}

}  // extern "C"
