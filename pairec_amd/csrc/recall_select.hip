// recall_select.hip — from candidate keys to the ordered answer of a recall: the ORDER BY distance desc LIMIT n of the searches
// recall.hip replaces (service/recall/hologres_vector_recall.go:23; FaissModel.Run, algorithm/faiss/model.go:29-31).
//   select_kernel    per query: radix-select the K-th largest key of the candidates, keep the top
//                    K, publish the new threshold (any K-th-largest-so-far is a valid lower bound,
//                    so the result is exact for every data distribution).
//   final_kernel     per query: bitonic sort of the K survivors in LDS, decode to (row, score); final_kernel_reg,
//                    final_rank_kernel and the split sort (FinalSortPolicy) are its faster forms, chosen by final_launch.
//   merge_keys_kernel + select + final: the global top-k of per-shard lists (topk_merge_*_locked, pg_topk_merge_dev).
// Called by the table pass (recall.hip) and by index_search.hip, group.hip, exclude.hip and cf.hip.
#include "common.hpp"
#include "recall_shared.hpp"
#include "bitonic_reg.hpp"
#include "split_sort.hpp"

namespace pg {

// ---------------------------------------------------------------------------------------------
// select: keep the K largest keys of cand_in[q][0..M) in cand_out[q][0..min(M,K)), set cnt, thr.
// One 1024-thread workgroup per query; 8 radix passes (one byte each) over L2-resident keys.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kSelLdsKeys = 16384;          // candidate lists up to this size are selected in LDS

// Block-wide radix-select helper state lives in LDS; keys come from `src` (LDS or global).
__global__ __launch_bounds__(1024) void select_kernel(const uint64_t* __restrict__ cand_in,
                                                      uint64_t* __restrict__ cand_out,
                                                      uint32_t* __restrict__ cnt,
                                                      float* __restrict__ thr, uint32_t cap,
                                                      uint32_t K, int thr_only, uint32_t* __restrict__ cnt_seen) {
    // thr_only: the lists stay as they are (cand_out is not written, cnt unchanged); the query's threshold rises to the
    // score of its K-th largest candidate so far — when it has that many (the refinement step of the pilot plan)
    extern __shared__ __attribute__((aligned(16))) char sel_smem[];
    uint64_t* const lkeys = reinterpret_cast<uint64_t*>(sel_smem);          // [kSelLdsKeys] when used
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_digit, s_need, s_out, s_cnt;
    __shared__ unsigned long long s_min, s_max;
    const uint32_t q = blockIdx.x;
    const uint64_t* in = cand_in + (uint64_t)q * cap;
    uint64_t* out = cand_out + (uint64_t)q * cap;
    uint32_t M = cnt[q];
    if (threadIdx.x == 0 && cnt_seen) cnt_seen[q] = M;      // (statistics: the candidates collected before K of them are kept)
    if (M > cap) M = cap;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_min = ~0ull; s_max = 0ull; }
    __syncthreads();
    const bool in_lds = M <= kSelLdsKeys;
    // pass 0: stage the keys in LDS (when they fit) and find their range
    unsigned long long mn = ~0ull, mx = 0ull;
    for (uint32_t i = tid; i < M; i += 1024) {
        const uint64_t k = in[i];
        if (in_lds) lkeys[i] = k;
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    }
    // wave-level reduce, then one LDS atomic per wave
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long omn = __shfl_xor(mn, off), omx = __shfl_xor(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
    }
    if ((tid & 63) == 0) {
        atomicMin(&s_min, mn);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    const uint64_t kmin = s_min, kmax = s_max;
    const uint64_t* src = in_lds ? lkeys : in;
    if (M <= K) {
        if (!thr_only)
            for (uint32_t i = tid; i < M; i += 1024) out[i] = src[i];
        if (tid == 0) {
            if (!thr_only) cnt[q] = M;
            if (M == K && K > 0) thr[q] = key_score(kmin);     // threshold = score of the smallest key
        }
        return;
    }
    // radix select of the K-th largest of (key - kmin): only the bits below the span's top bit vary,
    // so the first digit is already well spread (no single hot histogram bin)
    const uint64_t span = kmax - kmin;
    int shift = span ? (63 - __clzll((long long)span)) - 7 : 0;
    if (shift < 0) shift = 0;
    uint64_t prefix = 0, mask = 0;              // over (key - kmin)
    uint32_t need = K;
    uint32_t bucket = M;
    while (true) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < M; i += 1024) {
            const uint64_t k = src[i] - kmin;
            if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t above = 0;
            for (int d = 255; d > (int)tid; --d) above += hist[d];
            if (above < need && need <= above + hist[tid]) {
                s_digit = tid;
                s_need = need - above;
                s_cnt = hist[tid];
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_digit << shift;
        mask |= 255ull << shift;
        need = s_need;
        bucket = s_cnt;
        __syncthreads();
        if (shift == 0 || bucket == 1) break;
        shift = shift >= 8 ? shift - 8 : 0;
    }
    // keys are distinct.  If the selected bucket holds one key, that key is the K-th; otherwise all
    // digits down to bit 0 were fixed and prefix is the full (key - kmin) of the K-th.
    if (shift != 0) {
        if (tid == 0) s_min = 0ull;
        __syncthreads();
        for (uint32_t i = tid; i < M; i += 1024) {
            const uint64_t k = src[i] - kmin;
            if ((k & mask) == prefix) s_min = k;            // exactly one thread writes
        }
        __syncthreads();
        prefix = s_min;
    }
    const uint64_t kth = prefix + kmin;          // exactly K keys are >= kth
    if (thr_only) {
        if (tid == 0) thr[q] = key_score(kth);
        return;
    }
    if (tid == 0) s_out = 0;
    __syncthreads();
    for (uint32_t i = tid; i < M; i += 1024) {
        const uint64_t k = src[i];
        if (k >= kth) out[atomicAdd(&s_out, 1u)] = k;
    }
    if (tid == 0) {
        cnt[q] = K;
        thr[q] = key_score(kth);
    }
}

// final: sort the survivors descending in LDS and decode.  P = pow2 >= n, P*8 bytes of LDS.
__global__ __launch_bounds__(1024) void final_kernel(const uint64_t* __restrict__ cand,
                                                     const uint32_t* __restrict__ cnt, uint32_t cap,
                                                     uint32_t K, uint32_t P, uint64_t row_offset,
                                                     uint64_t* __restrict__ out_rows,
                                                     float* __restrict__ out_scores,
                                                     uint32_t* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint64_t* s = reinterpret_cast<uint64_t*>(smem_raw);
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t n = cnt[q];
    if (n > K) n = K;
    const uint64_t* in = cand + (uint64_t)q * cap;
    for (uint32_t i = tid; i < P; i += 1024) s[i] = i < n ? in[i] : 0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t idx = tid; idx < P; idx += 1024) {
                const uint32_t ixj = idx ^ j;
                if (ixj > idx) {
                    const uint64_t x = s[idx], y = s[ixj];
                    const bool desc = (idx & k) == 0;
                    if ((x < y) == desc) {
                        s[idx] = y;
                        s[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < K; i += 1024) {
        if (i < n) {
            out_rows[(uint64_t)q * K + i] = row_offset + key_row(s[i]);
            out_scores[(uint64_t)q * K + i] = key_score(s[i]);
        } else {
            out_rows[(uint64_t)q * K + i] = ~0ull;
            out_scores[(uint64_t)q * K + i] = -__builtin_inff();
        }
    }
    if (tid == 0 && out_count) out_count[q] = n;
}

// final for K <= 8192: the register-resident bitonic network (bitonic_reg.hpp) on complemented keys
__global__ __launch_bounds__(1024) void final_kernel_reg(const uint64_t* __restrict__ cand,
                                                         const uint32_t* __restrict__ cnt, uint32_t cap,
                                                         uint32_t K, uint64_t row_offset,
                                                         uint64_t* __restrict__ out_rows,
                                                         float* __restrict__ out_scores,
                                                         uint32_t* __restrict__ out_count) {
    __shared__ BitonicLds lds;
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    uint32_t n = cnt[q];
    if (n > K) n = K;
    uint32_t P = 512;
    while (P < K) P <<= 1;
    const uint64_t* in = cand + (uint64_t)q * cap;
    uint64_t k[kBitonicE];
    uint32_t ix[kBitonicE];
#pragma unroll
    for (int u = 0; u < kBitonicE; ++u) {
        const uint32_t i = t * kBitonicE + u;
        k[u] = (i < n) ? ~in[i] : ~0ull;               // descending = ascending on the complement; pad last
        ix[u] = 0;
    }
    bitonic_sort_reg<false>(k, ix, P, lds, n);
#pragma unroll
    for (int u = 0; u < kBitonicE; ++u) {
        const uint32_t i = t * kBitonicE + u;
        if (i < K) {
            const uint64_t key = ~k[u];
            if (i < n) {
                out_rows[(uint64_t)q * K + i] = row_offset + key_row(key);
                out_scores[(uint64_t)q * K + i] = key_score(key);
            } else {
                out_rows[(uint64_t)q * K + i] = ~0ull;
                out_scores[(uint64_t)q * K + i] = -__builtin_inff();
            }
        }
    }
    if (t == 0 && out_count) out_count[q] = n;
}

// final for a handful of queries (K <= 8192): counting ranks instead of a sorting network.  One workgroup sorts a
// query's 8192-slot network on ONE CU in 48 us whatever the chip is doing; with only a few queries in the call the
// other 250 CUs are idle, so every 64 candidates get a workgroup of their own: it stages the query's n keys in LDS
// (broadcast reads), wave p counts the keys above each of its 64 within the p-th quarter, the four counts add up
// to the candidate's rank — its output position, the keys being distinct.  n^2 / 4 compares per wave: ~6 us at 5 000.
// EPB candidates per workgroup, 256 / EPB threads each: 16 for one or two queries, 64 beyond.
template <int EPB>
__global__ __launch_bounds__(256) void final_rank_kernel(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ cnt,
                                                         uint32_t cap, uint32_t K, uint64_t row_offset,
                                                         uint64_t* __restrict__ out_rows, float* __restrict__ out_scores,
                                                         uint32_t* __restrict__ out_count) {
    constexpr uint32_t PARTS = 256 / EPB;
    extern __shared__ __attribute__((aligned(16))) uint64_t rk_keys[];       // [n rounded up to 32]
    __shared__ uint32_t part[PARTS][EPB];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    uint32_t n = cnt[q];
    if (n > K) n = K;
    // positions past the candidates (fewer than K rows in the table)
    for (uint32_t i = n + blockIdx.x * 256u + tid; i < K; i += gridDim.x * 256u) {
        out_rows[(uint64_t)q * K + i] = ~0ull;
        out_scores[(uint64_t)q * K + i] = -__builtin_inff();
    }
    if (blockIdx.x == 0 && tid == 0 && out_count) out_count[q] = n;
    if (blockIdx.x * (uint32_t)EPB >= n) return;
    const uint64_t* in = cand + (uint64_t)q * cap;
    const uint32_t n8 = (n + 31u) & ~31u;
    for (uint32_t i0 = tid; i0 < n8; i0 += 8u * 256u) {                     // eight independent loads per thread in flight
        uint64_t kv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t i = i0 + (uint32_t)u * 256u;
            kv[u] = in[i < n ? i : 0u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t i = i0 + (uint32_t)u * 256u;
            if (i < n8) rk_keys[i] = i < n ? kv[u] : 0ull;                  // padding: below every real key
        }
    }
    __syncthreads();
    const uint32_t el = tid % (uint32_t)EPB, p = tid / (uint32_t)EPB;
    const uint32_t e = blockIdx.x * (uint32_t)EPB + el;
    const uint64_t mine = e < n ? rk_keys[e] : ~0ull;
    const uint32_t chunk = n8 / PARTS;                                     // n8 % 32 == 0: even chunks
    const uint32_t j0 = p * chunk, j1 = j0 + chunk;
    uint32_t above = 0;
    // (unrolled: one wave per SIMD here, so a broadcast read's LDS latency is hidden only by the reads behind it)
#pragma unroll 4
    for (uint32_t j = j0; j < j1; j += 2) {
        const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(&rk_keys[j]);
        above += (kk.x > mine) ? 1u : 0u;
        above += (kk.y > mine) ? 1u : 0u;
    }
    part[p][el] = above;
    __syncthreads();
    if (p == 0 && e < n) {
        uint32_t r = 0;
#pragma unroll
        for (uint32_t i = 0; i < PARTS; ++i) r += part[i][el];
        out_rows[(uint64_t)q * K + r] = row_offset + key_row(mine);
        out_scores[(uint64_t)q * K + r] = key_score(mine);
    }
}

// merge input lists (global rows, scores) → candidate keys.  Padding entries (row = UINT64_MAX: a shard with fewer
// than per_list rows) are dropped here, so the keys stay distinct (select_kernel's invariant) and cnt[q] is the number
// of real candidates.  Input layout: [nq][nlists][per_list] (list_major = 0) or [nlists][nq][per_list] (1: what an
// all-gather of per-shard [nq][per_list] blocks produces).  cnt must be zero on entry.
// list l of query q starts at rows + l * row_ls + q * row_qs (scores likewise): covers the query-major layout
// [nq][nlists][per_list], the list-major one an all-gather produces, and packed per-shard (rows | scores) blocks
__global__ void merge_keys_kernel(const uint64_t* __restrict__ rows, const float* __restrict__ scores, uint32_t nq,
                                  uint32_t nlists, uint32_t per_list, size_t row_ls, size_t row_qs, size_t sc_ls, size_t sc_qs,
                                  uint32_t cap, uint64_t* __restrict__ cand, uint32_t* __restrict__ cnt) {
    const uint32_t q = blockIdx.y;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per_q = nlists * per_list;
    if (i >= per_q) return;
    const uint32_t l = i / per_list, j = i - l * per_list;
    const uint64_t r = rows[l * row_ls + q * row_qs + j];
    if (r == ~0ull) return;
    cand[(uint64_t)q * cap + atomicAdd(&cnt[q], 1u)] = topk_key(scores[l * sc_ls + q * sc_qs + j], (uint32_t)r);
}

int launch_select(pg_ctx* ctx, uint32_t nq, const uint64_t* in, uint64_t* out, uint32_t* cnt, float* thr,
                         uint32_t cap, uint32_t k, int thr_only, uint32_t* cnt_seen) {
    constexpr size_t lds = (size_t)kSelLdsKeys * 8;
    int rc_attr;
    if ((rc_attr = ensure_dyn_lds(ctx, (const void*)select_kernel, lds))) return rc_attr;
    select_kernel<<<nq, 1024, lds, ctx->stream>>>(in, out, cnt, thr, cap, k, thr_only, cnt_seen);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// final as a split sort (split_sort.hpp): descending by candidate key = ascending on the complement, keys distinct
struct FinalSortPolicy {
    static constexpr bool kWithIdx = false;
    const uint64_t* cand;
    const uint32_t* cnt;
    uint32_t cap, K;
    uint64_t row_offset;
    uint64_t* out_rows;
    float* out_scores;
    uint32_t* out_count;
    __device__ uint32_t count(uint32_t q) const { const uint32_t n = cnt[q]; return n < K ? n : K; }
    __device__ uint64_t key(uint32_t q, uint32_t i) const { return ~cand[(uint64_t)q * cap + i]; }
    __device__ void store(uint32_t q, uint32_t rank, uint64_t k, uint32_t) const {
        out_rows[(uint64_t)q * K + rank] = row_offset + key_row(~k);
        out_scores[(uint64_t)q * K + rank] = key_score(~k);
    }
    // positions past the candidates (fewer than K rows in the table); t = this thread among nt of the list's workgroups
    __device__ void tail(uint32_t q, uint32_t n, uint32_t t, uint32_t nt) const {
        for (uint32_t i = n + t; i < K; i += nt) {
            out_rows[(uint64_t)q * K + i] = ~0ull;
            out_scores[(uint64_t)q * K + i] = -__builtin_inff();
        }
        if (t == 0 && out_count) out_count[q] = n;
    }
};

int final_launch(pg_ctx* ctx, const uint64_t* cand, const uint32_t* cnt, uint32_t cap,
                        uint32_t nq, uint32_t k, uint64_t row_offset, uint64_t* d_out_rows,
                        float* d_out_scores, uint32_t* d_out_count) {
    if (!rank_sort_applies(ctx, nq, k, 1.5) && split_sort_applies(ctx, nq, k))
        return split_sort_launch(ctx, FinalSortPolicy{cand, cnt, cap, k, row_offset, d_out_rows, d_out_scores, d_out_count}, nq, k);
    if (rank_sort_applies(ctx, nq, k, 1.5)) {
        const size_t lds = (size_t)((k + 31u) & ~31u) * 8;
        int rc_attr;
        if (nq <= 2) {
            if ((rc_attr = ensure_dyn_lds(ctx, (const void*)final_rank_kernel<16>, lds))) return rc_attr;
            final_rank_kernel<16><<<dim3((k + 15) / 16, nq), 256, lds, ctx->stream>>>(cand, cnt, cap, k, row_offset, d_out_rows,
                                                                                      d_out_scores, d_out_count);
        } else {
            if ((rc_attr = ensure_dyn_lds(ctx, (const void*)final_rank_kernel<64>, lds))) return rc_attr;
            final_rank_kernel<64><<<dim3((k + 63) / 64, nq), 256, lds, ctx->stream>>>(cand, cnt, cap, k, row_offset, d_out_rows,
                                                                                      d_out_scores, d_out_count);
        }
        PG_HIP(hipGetLastError());
        return PG_OK;
    }
    if (k <= kBitonicMax) {
        final_kernel_reg<<<nq, 1024, 0, ctx->stream>>>(cand, cnt, cap, k, row_offset, d_out_rows, d_out_scores,
                                                       d_out_count);
        PG_HIP(hipGetLastError());
        return PG_OK;
    }
    const uint32_t P = next_pow2(k < 2 ? 2 : k);
    const size_t lds = (size_t)P * 8;
    int rc_attr;
    if ((rc_attr = ensure_dyn_lds(ctx, (const void*)final_kernel, lds))) return rc_attr;
    final_kernel<<<nq, 1024, lds, ctx->stream>>>(cand, cnt, cap, k, P, row_offset, d_out_rows,
                                                 d_out_scores, d_out_count);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int topk_merge_strided_locked(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t nlists,
                              uint32_t per_list, size_t row_ls, size_t row_qs, size_t sc_ls, size_t sc_qs, uint32_t k,
                              uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count) {
    if (nq < 1 || nq > (uint32_t)kMaxQueries) {
        set_error("topk merge: nq=%u out of range", nq);
        return PG_ERR_INVALID;
    }
    const uint64_t per_q = (uint64_t)nlists * per_list;
    if (k < 1 || k > 16384 || per_q == 0 || per_q > k + kCandSlack) {
        set_error("topk merge: unsupported sizes k=%u lists=%u x %u", k, nlists, per_list);
        return PG_ERR_UNSUPPORTED;
    }
    RecallScratch rs;
    int rc;
    if ((rc = recall_scratch(ctx, 64, k, &rs))) return rc;
    PG_HIP(hipMemsetAsync(rs.cnt, 0, sizeof(uint32_t) * kMaxQueries, ctx->stream));
    dim3 grid((uint32_t)((per_q + 255) / 256), nq);
    merge_keys_kernel<<<grid, 256, 0, ctx->stream>>>(d_rows, d_scores, nq, nlists, per_list, row_ls, row_qs, sc_ls, sc_qs, rs.cap, rs.cand[0],
                                                    rs.cnt);
    PG_HIP(hipGetLastError());
    if ((rc = launch_select(ctx, nq, rs.cand[0], rs.cand[1], rs.cnt, rs.thr, rs.cap, k, 0))) return rc;
    return final_launch(ctx, rs.cand[1], rs.cnt, rs.cap, nq, k, 0, d_out_rows, d_out_scores, d_out_count);
}

// global top-k of nlists per-shard lists per query (identical and deterministic on every shard that runs it)
int topk_merge_locked(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t nlists,
                      uint32_t per_list, int list_major, uint32_t k, uint64_t* d_out_rows, float* d_out_scores,
                      uint32_t* d_out_count) {
    const size_t ls = list_major ? (size_t)nq * per_list : (size_t)per_list;
    const size_t qs = list_major ? (size_t)per_list : (size_t)nlists * per_list;
    return topk_merge_strided_locked(ctx, d_rows, d_scores, nq, nlists, per_list, ls, qs, ls, qs, k, d_out_rows, d_out_scores, d_out_count);
}

}  // namespace pg

extern "C" {

int pg_topk_merge_dev(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq,
                      uint32_t nlists, uint32_t per_list, uint32_t k, uint64_t* d_out_rows,
                      float* d_out_scores) {
    PG_REQUIRE(ctx && d_rows && d_scores && d_out_rows && d_out_scores, "pg_topk_merge_dev: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    return pg::topk_merge_locked(ctx, d_rows, d_scores, nq, nlists, per_list, 0, k, d_out_rows, d_out_scores, nullptr);
}

}  // extern "C"
