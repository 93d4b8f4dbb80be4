// index_build.hip — building and refreshing an exact IVF index, all on the device.
//
// Build: k-means over a sample of the rows (Lloyd, deterministic centroid sums in fp64), every row assigned to its nearest
// centroid, a stable sort by list into a uint32 permutation (rows of one list in ascending source order) with the lists'
// offsets, a per-list radius r_L >= max ||x - c_L|| over the rows actually assigned (fp64, rounded up) and ||c_L||.
// Refresh (pg_index_refresh): the centroids stay; the rows of the table's write log, or all rows, are re-assigned by the same
// rule, and the build's tail (lists_finish) makes the new permutation, offsets and radii in new arrays that are then exchanged
// for the old ones.
#include "index_shared.hpp"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>

namespace pg {
namespace {

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

// ---- an index's device arrays (IndexArrays, index_shared.hpp): THE layout, the allocation and the release ----------------
hipError_t index_arrays_free(IndexArrays* a) {      // (the first error, after both were tried)
    const hipError_t e0 = a->perm ? hipFree(a->perm) : hipSuccess, e1 = a->small ? hipFree(a->small) : hipSuccess;
    *a = IndexArrays{};
    return e0 != hipSuccess ? e0 : e1;
}

// index memory: the permutation and the per-list arrays (one allocation: off | cent | cnorm | rad, off and the two per-list
// arrays padded to 256 B).  PG_ERR_NOMEM leaves *a empty.
int index_arrays_alloc(IndexArrays* a, uint64_t rows, uint32_t nl, uint32_t dim) {
    const size_t off_b = align_up((size_t)(nl + 1) * 4), cent_b = (size_t)nl * dim * 4, lists_b = align_up((size_t)nl * 4);
    int rc;
    if ((rc = dalloc((void**)&a->perm, rows * 4)) || (rc = dalloc(&a->small, off_b + cent_b + 2 * lists_b))) {
        (void)index_arrays_free(a);
        return rc;
    }
    a->off = (uint32_t*)a->small;
    a->cent = (float*)((char*)a->small + off_b);
    a->cnorm = (float*)((char*)a->cent + cent_b);
    a->rad = (float*)((char*)a->cnorm + lists_b);
    return PG_OK;
}

// What a build and a refresh end with, once the rows' lists (assign) are known: the stable sort by list is to.perm with its
// offsets to.off, the radii to.rad over the rows actually assigned (to.cent: the centroids, already in place); then the radii,
// the offsets and the 4 flag words (flag[0]: a non-finite row) on the host.  Synchronises.
struct ListFigures {
    std::vector<float> rad;
    std::vector<uint32_t> off;
    uint32_t flag[4] = {0, 0, 0, 0};
};
int lists_finish(pg_ctx* ctx, const pg_table* t, uint64_t rows, uint32_t nl, const uint32_t* assign, uint32_t* keys_s, uint32_t* vals_in, const IndexArrays& to,
                 void* tmp, size_t tmp_bytes, const uint32_t* flag, ListFigures* out) {
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = sort_by_list(ctx, assign, rows, nl, keys_s, vals_in, to.perm, to.off, tmp, tmp_bytes))) return rc;
    PG_HIP(hipMemsetAsync(to.rad, 0, (size_t)nl * 4, s));
    radius_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(t->d, rows, t->dim, assign, to.cent, (uint32_t*)to.rad);
    PG_HIP(hipGetLastError());
    out->rad.resize(nl);
    out->off.resize((size_t)nl + 1);
    PG_HIP(hipMemcpyAsync(out->rad.data(), to.rad, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipMemcpyAsync(out->off.data(), to.off, ((size_t)nl + 1) * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipMemcpyAsync(out->flag, flag, 16, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    return PG_OK;
}

// (ix->a is the caller's to release when this fails)
int index_build_locked(pg_ctx* ctx, const pg_table* t, const pg_index_params& p, pg_index* ix, std::vector<void*>& temp) {
    const uint64_t rows = t->rows;
    const uint32_t dim = t->dim;
    const IndexBuildShape shape = index_build_shape(rows, p);
    const uint32_t nl = shape.n_lists, iters = shape.iters;
    const uint64_t ns = shape.train_rows;
    ix->n_lists = nl;
    int rc;
    if ((rc = index_arrays_alloc(&ix->a, rows, nl, dim))) return rc;
    const IndexArrays& a = ix->a;
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
    vals_s = a.perm;                         // (the sample's sort uses the permutation's memory before the table's does)
    PG_HIP(hipMemsetAsync(flag, 0, 16, ctx->stream));
    // 1. the sample: rows (mul * i + add) mod rows, mul coprime to rows; the first n_lists of them seed the centroids
    uint64_t sx = p.seed ^ 0x1D8E4E27C47D124Full;
    uint64_t mul = rows > 1 ? 1 + splitmix(sx) % (rows - 1) : 1;
    while (gcd64(mul, rows) != 1) mul = mul + 1 < rows ? mul + 1 : 1;
    const uint64_t add = splitmix(sx) % rows;
    sample_gather_kernel<<<(uint32_t)ns, 64, 0, ctx->stream>>>(t->d, rows, dim, mul, add, S);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(a.cent, S, (size_t)nl * dim * 4, hipMemcpyDeviceToDevice, ctx->stream));
    // 2. Lloyd iterations over the sample
    for (uint32_t it = 0; it < iters; ++it) {
        if ((rc = assign_dispatch(ctx, dim, S, ns, a.cent, cn2, nl, assign, flag + 1))) return rc;
        if ((rc = sort_by_list(ctx, assign, ns, nl, keys_s, vals_in, vals_s, soff, tmp, tmp_bytes))) return rc;
        centroid_update_kernel<<<nl, 64, 0, ctx->stream>>>(S, (uint32_t)ns, dim, vals_s, soff, a.cent, splitmix(sx));
        PG_HIP(hipGetLastError());
    }
    // 3. every row to its nearest centroid, 4. centroid norms
    if ((rc = assign_dispatch(ctx, dim, t->d, rows, a.cent, cn2, nl, assign, flag))) return rc;
    cnorm_kernel<<<(nl + 255) / 256, 256, 0, ctx->stream>>>(a.cent, nl, dim, a.cnorm);
    PG_HIP(hipGetLastError());
    // 5. the stable sort by list is the permutation; radii over the rows actually assigned
    ListFigures fig;
    if ((rc = lists_finish(ctx, t, rows, nl, assign, keys_s, vals_in, a, tmp, tmp_bytes, flag, &fig))) return rc;
    ix->nonfinite = fig.flag[0] != 0;
    ix->st.n_lists = nl;
    ix->st.dim = dim;
    ix->st.rows = rows;
    list_summary(fig.rad, fig.off, &ix->st);
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
    IndexArrays a;
    ListFigures fig;                     // (flag[0]: a non-finite row; flag[2, 4): the rows whose list changed)
    uint64_t reassigned = 0, moved = 0, wide = 0;
    double assign_ms = 0.0;
};

// The new permutation, offsets and radii of ix for the table's current rows and ix's centroids, in new buffers; caller holds
// ctx->mu and the table's shared lock.  incremental: only the rows of the table's write log are re-assigned.
int index_refresh_locked(pg_ctx* ctx, const pg_index* ix, bool incremental, RefreshOut* o, std::vector<void*>& temp,
                         hipEvent_t ev0, hipEvent_t ev1) {
    const pg_table* t = ix->t;
    const uint64_t rows = ix->rows;
    const uint32_t dim = ix->dim, nl = ix->n_lists;
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = index_arrays_alloc(&o->a, rows, nl, dim))) return rc;
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
    PG_HIP(hipMemcpyAsync(o->a.cent, ix->a.cent, (size_t)nl * dim * 4, hipMemcpyDeviceToDevice, s));
    PG_HIP(hipMemcpyAsync(o->a.cnorm, ix->a.cnorm, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
    // the lists the index holds now, per row (the full path counts the moved rows against them)
    uint32_t* const old_assign = incremental ? assign : vals_in;
    list_of_row_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(ix->a.perm, ix->a.off, rows, nl, old_assign);
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
        if ((rc = reassign_rows(ctx, t, ix->a.cent, cn2, nl, ids, d_rows, xg, vals, assign, flag, moved))) return rc;
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
            rc = assign_screen_launch(ctx, dim, t->d, rows, ix->a.cent, nl, ws, assign, wide, flag + 1, flag);
            if (rc == PG_OK) {
                screened = true;
                uint32_t h_wide = 0;
                PG_HIP(hipMemcpyAsync(&h_wide, flag + 1, 4, hipMemcpyDeviceToHost, s));
                PG_HIP(hipStreamSynchronize(s));
                // the rows the screen left open: the fp32 kernel against all lists (`assign` holds nothing for them yet: the
                // moved rows are counted against old_assign below)
                if ((rc = reassign_rows(ctx, t, ix->a.cent, cn2, nl, wide, h_wide, xg, vals, assign, flag, nullptr))) return rc;
                o->wide = h_wide;
            } else if (rc != PG_ERR_UNSUPPORTED) {
                return rc;
            }
        }
        // (a centroid outside the screen's range, dim 192 / 256: the fp32 kernel for every row)
        if (!screened && (rc = assign_dispatch(ctx, dim, t->d, rows, ix->a.cent, cn2, nl, assign, flag))) return rc;
        count_moved_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(old_assign, assign, rows, moved);
        PG_HIP(hipGetLastError());
        o->reassigned = rows;
    }
    PG_HIP(hipEventRecord(ev1, s));
    // the build's tail: the stable sort by list is the permutation, offsets, radii over the rows actually assigned
    if ((rc = lists_finish(ctx, t, rows, nl, assign, keys_s, vals_in, o->a, tmp, tmp_bytes, flag, &o->fig))) return rc;
    memcpy(&o->moved, o->fig.flag + 2, 8);
    float ms = 0.0f;
    PG_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    o->assign_ms = ms;
    return PG_OK;
}

}  // namespace
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
    std::vector<void*> temp;
    int rc = pg::index_build_locked(ctx, t, params, ix, temp);
    if (rc == PG_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        pg::set_error("pg_index_build: %s", hipGetErrorString(hipGetLastError()));
        rc = PG_ERR_DEVICE;
    }
    if (rc != PG_OK) (void)hipStreamSynchronize(ctx->stream);
    pg::free_all(temp);
    if (rc != PG_OK) {
        if (rc == PG_ERR_NOMEM) pg::set_error("pg_index_build: device allocation failed (%llu rows x %u)", (unsigned long long)t->rows, t->dim);
        (void)pg::index_arrays_free(&ix->a);
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
    const pg::RefreshPlan plan = pg::refresh_plan(prm.mode, covered, logged, ix->rows, ctx->knobs.index_refresh_full_fraction, gen == ix->gen);
    if (plan == pg::RefreshPlan::refused) {
        pg::set_error("pg_index_refresh: the table's write log starts at generation %llu, the index describes %llu (refresh in full)",
                      (unsigned long long)t->log_since, (unsigned long long)ix->gen);
        return PG_ERR_UNSUPPORTED;
    }
    const bool incremental = plan == pg::RefreshPlan::incremental;
    PG_HIP(hipSetDevice(ctx->device));
    hipEvent_t ev[2] = {nullptr, nullptr};
    PG_HIP(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) {
        (void)hipEventDestroy(ev[0]);
        pg::set_error("pg_index_refresh: %s", hipGetErrorString(hipGetLastError()));
        return PG_ERR_DEVICE;
    }
    pg::RefreshOut o;
    std::vector<void*> temp;
    int rc = pg::index_refresh_locked(ctx, ix, incremental, &o, temp, ev[0], ev[1]);
    if (rc != PG_OK) (void)hipStreamSynchronize(ctx->stream);
    pg::free_all(temp);
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    if (rc != PG_OK) {
        if (rc == PG_ERR_NOMEM) pg::set_error("pg_index_refresh: device allocation failed (%llu rows x %u)", (unsigned long long)ix->rows, ix->dim);
        (void)pg::index_arrays_free(&o.a);
        return rc;                           // (the index as it was: stale and valid)
    }
    // install as pg_index_attach replaces an index: the table exclusively (no generation bump), the device drained so that no
    // enqueued index plan reads the old arrays, then the exchange.  A write between the two locks leaves the index stale again.
    tr.unlock();
    {
        std::unique_lock<std::shared_mutex> w(t->rw);
        if (hipDeviceSynchronize() != hipSuccess) {
            pg::set_error("pg_index_refresh: %s", hipGetErrorString(hipGetLastError()));
            (void)pg::index_arrays_free(&o.a);
            return PG_ERR_DEVICE;
        }
        std::swap(ix->a, o.a);               // (o.a: the old arrays from here on)
        ix->gen = gen;
        ix->nonfinite = o.fig.flag[0] != 0;
        {
            std::lock_guard<std::mutex> gw(ix->where_mu);       // (the cached filters' keys carry the old generation)
            pg::where_cache_clear(ix->where_cache, ix->where_st);
        }
        std::lock_guard<std::mutex> gs(ix->mu);
        ix->st.generation = gen;
        pg::list_summary(o.fig.rad, o.fig.off, &ix->st);
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
    (void)pg::index_arrays_free(&o.a);
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
    PG_HIP(pg::index_arrays_free(&ix->a));
    delete ix;
    return PG_OK;
}

int pg_index_read(pg_ctx* ctx, const pg_index* ix, uint32_t* offsets, uint32_t* perm, float* centroids, float* cnorm, float* radius) {
    PG_REQUIRE(ctx && ix, "pg_index_read: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);             // (pg_index_refresh exchanges the arrays under the exclusive lock)
    hipStream_t s = ctx->stream;
    const size_t nl = ix->n_lists;
    if (offsets) PG_HIP(hipMemcpyAsync(offsets, ix->a.off, (nl + 1) * 4, hipMemcpyDeviceToHost, s));
    if (perm) PG_HIP(hipMemcpyAsync(perm, ix->a.perm, (size_t)ix->rows * 4, hipMemcpyDeviceToHost, s));
    if (centroids) PG_HIP(hipMemcpyAsync(centroids, ix->a.cent, nl * ix->dim * 4, hipMemcpyDeviceToHost, s));
    if (cnorm) PG_HIP(hipMemcpyAsync(cnorm, ix->a.cnorm, nl * 4, hipMemcpyDeviceToHost, s));
    if (radius) PG_HIP(hipMemcpyAsync(radius, ix->a.rad, nl * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    return PG_OK;
}

}  // extern "C"
