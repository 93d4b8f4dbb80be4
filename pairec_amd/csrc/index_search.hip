// index_search.hip — the search of an exact IVF index, per batch of queries:
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
// One launch sequence (index_search) serves both callers (index.hip).  After each stage's count a plan kernel writes the verdict
// — the dense rule, a non-finite query, the rounds the stage takes — into the plan words, and every round's expansion reads it.
#include "index_shared.hpp"

#include <cmath>

namespace pg {
namespace {

constexpr uint32_t kBoundQ = 8;          // queries per bound-kernel block

__device__ __forceinline__ uint32_t ukey(float f) {      // order-preserving bits (totalOrder for non-NaN)
    const uint32_t b = __float_as_uint(f);
    if (f != f) return 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
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

// the bounds of a batch: qn[q] >= ||q|| (and *flag |= 1 for a non-finite query), then U[q][L] — the one launch of the
// search and pg_index_bounds
int bounds_launch(pg_ctx* ctx, const pg_index* ix, const float* d_q, uint32_t nq, bool l2, double* qn, uint32_t* flag, float* U) {
    const uint32_t nl = ix->n_lists, dim = ix->dim;
    hipStream_t s = ctx->stream;
    qinfo_kernel<<<nq, 64, 0, s>>>(d_q, dim, qn, flag);
    const dim3 bg((nl + 255) / 256, (nq + kBoundQ - 1) / kBoundQ);
    const size_t blds = (size_t)kBoundQ * dim * 8;
    if (l2) bound_kernel<true><<<bg, 256, blds, s>>>(d_q, nq, dim, qn, ix->a.cent, ix->a.cnorm, ix->a.rad, nl, U);
    else bound_kernel<false><<<bg, 256, blds, s>>>(d_q, nq, dim, qn, ix->a.cent, ix->a.cnorm, ix->a.rad, nl, U);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace

// the layout of SearchBufs (index_shared.hpp)
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

}  // namespace pg

extern "C" {

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

}  // extern "C"
