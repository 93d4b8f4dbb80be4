// misc.hip — small glue kernels that keep a request batch on the device between stages.
#include "pipeline.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace pg {

// (uni_off != nullptr: the same launch also writes the uniform request offsets uni_off[r] = r * uni_k, r <= uni_nq <= n)
__global__ void rows_to_local_kernel(const uint64_t* __restrict__ rows, uint32_t n, uint64_t off,
                                     uint64_t nrows, uint32_t* __restrict__ local,
                                     uint8_t* __restrict__ owned, uint32_t* __restrict__ uni_off, uint32_t uni_nq, uint32_t uni_k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (uni_off && i <= uni_nq) uni_off[i] = i * uni_k;
    if (i >= n) return;
    const uint64_t r = rows[i];
    const bool mine = r != ~0ull && r >= off && r - off < nrows;
    local[i] = mine ? (uint32_t)(r - off) : 0u;
    if (owned) owned[i] = mine ? 1 : 0;
}

__global__ void widen_kernel(const float* __restrict__ in, uint32_t n, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

// read-only streaming probe: the measured HBM ceiling that bench.py reports beside the nominal 8 TB/s
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void hbm_probe_kernel(const u32x4* __restrict__ p, uint64_t n16,
                                                        uint32_t* __restrict__ sink) {
    uint32_t acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const u32x4 a = __builtin_nontemporal_load(&p[i]);
        const u32x4 b = __builtin_nontemporal_load(&p[i + stride]);
        const u32x4 c = __builtin_nontemporal_load(&p[i + 2 * stride]);
        const u32x4 d = __builtin_nontemporal_load(&p[i + 3 * stride]);
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < n16; i += stride) {
        const u32x4 a = __builtin_nontemporal_load(&p[i]);
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
    }
    if (acc == 0x9E3779B9u) *sink = acc;      // never true in practice; keeps the loads alive
}

// req_offsets[r] = r * k (uniform candidate count per request)
__global__ void uniform_offsets_kernel(uint32_t nq, uint32_t k, uint32_t* __restrict__ off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nq) off[i] = i * k;
}

// DPP candidates of request q: the first C entries of its sorted list → global row and relevance (fused score)
__global__ void sorted_head_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ rows,
                                   const double* __restrict__ fused, uint32_t nq, uint32_t k, uint32_t C,
                                   uint64_t* __restrict__ c_rows, double* __restrict__ c_rel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * C) return;
    const uint32_t q = i / C, j = i - q * C;
    const size_t src = (size_t)q * k + order[(size_t)q * k + j];
    c_rows[i] = rows[src];
    c_rel[i] = fused[src];
}

// the embedding rows this table holds among `c_rows` → out [n][dim] (16-B stores; out may live on a peer device)
__global__ void gather_global_rows_kernel(const float* __restrict__ tab, uint32_t dim, uint64_t off, uint64_t nrows,
                                          const uint64_t* __restrict__ c_rows, uint32_t n, float* __restrict__ out) {
    const uint32_t qpr = dim / 4;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = gid / qpr;
    const uint32_t c = (uint32_t)(gid % qpr);
    if (i >= n) return;
    const uint64_t r = c_rows[i];
    if (r == ~0ull || r < off || r - off >= nrows) return;
    *reinterpret_cast<float4*>(out + i * dim + 4 * c) = *reinterpret_cast<const float4*>(tab + (r - off) * dim + 4 * c);
}

// page[q][p] = entry pick[q][p] of request q's sorted list (pick = DPP's choice among the first C, or p itself)
__global__ void page_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ pick,
                            const uint32_t* __restrict__ pick_cnt, const uint64_t* __restrict__ rows,
                            const float* __restrict__ recall, const float* __restrict__ rank, size_t rank_stride, int n_algos,
                            const double* __restrict__ fused, uint32_t nq, uint32_t k, uint32_t top_n,
                            uint64_t* __restrict__ p_rows, double* __restrict__ p_fused,
                            float* __restrict__ p_recall, float* __restrict__ p_rank) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t np = nq * top_n;
    if (i >= np) return;
    const uint32_t q = i / top_n, p = i - q * top_n;
    uint32_t j = p;
    bool valid = true;
    if (pick) {
        valid = p < pick_cnt[q];
        j = valid ? pick[(size_t)q * top_n + p] : 0u;
    }
    const size_t src = (size_t)q * k + order[(size_t)q * k + j];
    p_rows[i] = valid ? rows[src] : ~0ull;
    p_fused[i] = valid ? fused[src] : __longlong_as_double(0x7FF8000000000000ll);
    p_recall[i] = valid ? recall[src] : -__builtin_inff();
    for (int a = 0; a < n_algos; ++a) p_rank[(size_t)a * np + i] = valid ? rank[(size_t)a * rank_stride + src] : 0.0f;
}

int sorted_head_launch(hipStream_t st, const uint32_t* d_order, const uint64_t* d_rows, const double* d_fused, uint32_t nq,
                       uint32_t k, uint32_t C, uint64_t* d_c_rows, double* d_c_rel) {
    if (nq == 0 || C == 0) return PG_OK;
    sorted_head_kernel<<<(nq * C + 255) / 256, 256, 0, st>>>(d_order, d_rows, d_fused, nq, k, C, d_c_rows, d_c_rel);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int gather_global_rows_launch(hipStream_t st, const pg_table* t, const uint64_t* d_global_rows, uint32_t n, float* d_out) {
    if (n == 0) return PG_OK;
    const uint64_t threads = (uint64_t)n * (t->dim / 4);
    gather_global_rows_kernel<<<(uint32_t)((threads + 255) / 256), 256, 0, st>>>(t->d, t->dim, t->row_offset, t->rows, d_global_rows, n, d_out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int page_launch(hipStream_t st, const uint32_t* d_order, const uint32_t* d_pick, const uint32_t* d_pick_cnt,
                const uint64_t* d_rows, const float* d_recall, const float* d_rank, size_t rank_stride, int n_algos,
                const double* d_fused, uint32_t nq, uint32_t k, uint32_t top_n, char* d_page) {
    const size_t np = (size_t)nq * top_n;
    if (np == 0) return PG_OK;
    const PageView page(d_page, np);
    page_kernel<<<(uint32_t)((np + 255) / 256), 256, 0, st>>>(d_order, d_pick, d_pick_cnt, d_rows, d_recall, d_rank, rank_stride, n_algos,
                                                             d_fused, nq, k, top_n, page.rows, page.fused, page.recall, page.rank);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int rows_to_local_locked(pg_ctx* ctx, const pg_table* t, const uint64_t* d_rows, uint32_t n, uint32_t* d_local,
                         uint8_t* d_owned) {
    if (n == 0) return PG_OK;
    rows_to_local_kernel<<<(n + 255) / 256, 256, 0, ctx->stream>>>(d_rows, n, t->row_offset, t->rows, d_local, d_owned, nullptr, 0, 0);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// rows_to_local_locked + uniform_offsets_locked in one launch (n = nq * k > nq)
int rows_to_local_offsets_locked(pg_ctx* ctx, const pg_table* t, const uint64_t* d_rows, uint32_t nq, uint32_t k, uint32_t* d_local,
                                 uint32_t* d_off) {
    const uint32_t n = nq * k;
    if (n <= nq) {
        int rc = uniform_offsets_locked(ctx, nq, k, d_off);
        return rc ? rc : rows_to_local_locked(ctx, t, d_rows, n, d_local, nullptr);
    }
    rows_to_local_kernel<<<(n + 255) / 256, 256, 0, ctx->stream>>>(d_rows, n, t->row_offset, t->rows, d_local, nullptr, d_off, nq, k);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int uniform_offsets_locked(pg_ctx* ctx, uint32_t nq, uint32_t k, uint32_t* d_off) {
    uniform_offsets_kernel<<<(nq + 256) / 256, 256, 0, ctx->stream>>>(nq, k, d_off);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_hbm_read_probe(pg_ctx* ctx, const pg_table* t, int reps, double* out_gbps) {
    PG_REQUIRE(ctx && t && out_gbps && reps > 0, "pg_hbm_read_probe: bad argument");
    const void* d_buf = t->d;
    const uint64_t bytes = t->rows * (uint64_t)t->dim * 4;
    PG_REQUIRE(bytes >= (1u << 20), "pg_hbm_read_probe: table smaller than 1 MiB");
    std::lock_guard<std::mutex> g(ctx->mu);
    void* sink;
    int rc;
    if ((rc = pg::scratch_reserve(ctx, pg::kSlotStatus, 4096, &sink))) return rc;
    const uint64_t n16 = bytes / 16;
    const int grid = ctx->num_cus * 8;
    double best = 0.0;
    for (int r = 0; r < reps + 1; ++r) {      // first launch is a warm-up
        PG_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
        pg::hbm_probe_kernel<<<grid, 256, 0, ctx->stream>>>((const pg::u32x4*)d_buf, n16, (uint32_t*)sink + 900);
        PG_HIP(hipGetLastError());
        PG_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        PG_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        const double gbps = (double)(n16 * 16) / (ms * 1e-3) / 1e9;
        if (r > 0 && gbps > best) best = gbps;
    }
    *out_gbps = best;
    return PG_OK;
}

int pg_rows_to_local_dev(pg_ctx* ctx, const pg_table* t, const uint64_t* d_rows, uint32_t n,
                         uint32_t* d_local, uint8_t* d_owned) {
    PG_REQUIRE(ctx && t && (n == 0 || (d_rows && d_local)), "pg_rows_to_local_dev: NULL argument");
    if (n == 0) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    return pg::rows_to_local_locked(ctx, t, d_rows, n, d_local, d_owned);
}

int pg_widen_f32_dev(pg_ctx* ctx, const float* d_in, uint32_t n, double* d_out) {
    PG_REQUIRE(ctx && (n == 0 || (d_in && d_out)), "pg_widen_f32_dev: NULL argument");
    if (n == 0) return PG_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::widen_kernel<<<(n + 255) / 256, 256, 0, ctx->stream>>>(d_in, n, d_out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // extern "C"
