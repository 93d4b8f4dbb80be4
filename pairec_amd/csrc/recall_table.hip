// recall_table.hip — what the table pass (recall.hip) derives from a table's rows, built lazily on first use and cached until
// the next upload / fill: the int8 / bf16 shadow and the statistics of the screen's bound (ensure_table_stats), |x|^2 of every
// row and the per-block minima of the squared-Euclidean recall (ensure_table_nx; service/recall/hologres_vector_recall_v2.go:23)
// and the threshold predictor's model (ensure_pred_model).  The builds are serialised by g_table_state_mu (table_state.hpp).
#include "common.hpp"
#include "recall_shared.hpp"

namespace pg {

// smallest |x|^2 of every 32-row block (rows past the table's end do not count)
// stats[0] += sum over rows of (|x|^2 - the block's smallest), stats[1] += sum of |x|^2: how much the per-block cutoff gives away
__global__ void block_nxmin_kernel(const float* __restrict__ nx, uint64_t rows, float* __restrict__ out, uint32_t nblocks,
                                   double* __restrict__ stats) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    double slack = 0.0, sum = 0.0;
    if (b < nblocks) {
        float m = __builtin_inff();
        bool nan = false;                            // (fminf skips a NaN: it has to be seen separately)
        for (uint32_t i = 0; i < (uint32_t)kPieceRows; ++i) {
            const uint64_t r = (uint64_t)b * kPieceRows + i;
            if (r < rows) {
                const float v = nx[r];
                nan |= v != v;
                m = fminf(m, v);
            }
        }
        m = nan ? 0.0f : m;                          // (a NaN norm: no help from this block)
        out[b] = m;
        for (uint32_t i = 0; i < (uint32_t)kPieceRows; ++i) {
            const uint64_t r = (uint64_t)b * kPieceRows + i;
            if (r < rows && nx[r] == nx[r] && nx[r] < 1e30f) { slack += (double)nx[r] - (double)m; sum += (double)nx[r]; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        slack += __shfl_xor(slack, off, 64);
        sum += __shfl_xor(sum, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && sum > 0.0) {
        atomicAdd(&stats[0], slack);
        atomicAdd(&stats[1], sum);
    }
}

// Table statistics without a shadow (first pass of the int8 build): max |x|, max row L2 norm^2, finiteness.
template <int DIM>
__global__ __launch_bounds__(256) void table_stats_kernel(const float* __restrict__ tab, uint64_t rows,
                                                          float* __restrict__ out_max, uint32_t* __restrict__ out_nonfinite,
                                                          float* __restrict__ out_absmax, float* __restrict__ out_sumsq) {
    constexpr int G = DIM / 8;
    __shared__ float smax[4], samax[4], ssum[4];
    __shared__ uint32_t sbad[4];
    const uint64_t n8 = rows * (uint64_t)G;
    float mx = 0.0f, amx = 0.0f, sum = 0.0f;
    uint32_t bad = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ((n8 + 63) & ~63ull);
         g += (uint64_t)gridDim.x * blockDim.x) {
        float ss = 0.0f;
        if (g < n8) {
            const float4 a = reinterpret_cast<const float4*>(tab)[2 * g];
            const float4 b = reinterpret_cast<const float4*>(tab)[2 * g + 1];
            ss = a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w + b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
            sum += ss;
            amx = fmaxf(amx, fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
                                   fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w)))));
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) ss += __shfl_xor(ss, off, 64);
        if (!(ss < 3.0e38f)) bad = 1;
        mx = fmaxf(mx, ss);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        amx = fmaxf(amx, __shfl_xor(amx, off, 64));
        sum += __shfl_xor(sum, off, 64);
        bad |= (uint32_t)__shfl_xor((int)bad, off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smax[w] = mx; samax[w] = amx; ssum[w] = sum; sbad[w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(reinterpret_cast<uint32_t*>(out_max), __float_as_uint(fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]))));
        atomicMax(reinterpret_cast<uint32_t*>(out_absmax),
                  __float_as_uint(fmaxf(fmaxf(samax[0], samax[1]), fmaxf(samax[2], samax[3]))));
        if (sbad[0] | sbad[1] | sbad[2] | sbad[3]) atomicOr(out_nonfinite, 1u);
        atomicAdd(out_sumsq, ssum[0] + ssum[1] + ssum[2] + ssum[3]);     // (statistics only: decides int8 vs bf16)
    }
}

// Second pass: the int8 shadow X = clamp(rint(x / s), +-127) and the largest row residual ||x - s X||^2.
// A thread converts 8 consecutive values (one 8-byte store); DIM/8 neighbouring lanes share a row.
template <int DIM>
__global__ __launch_bounds__(256) void table_quant8_kernel(const float* __restrict__ tab, uint64_t rows, float s,
                                                           int8_t* __restrict__ out8, float* __restrict__ out_resid) {
    constexpr int G = DIM / 8;
    __shared__ float smax[4];
    const uint64_t n8 = rows * (uint64_t)G;
    const float inv = 1.0f / s;
    float mx = 0.0f;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ((n8 + 63) & ~63ull);
         g += (uint64_t)gridDim.x * blockDim.x) {
        float rs = 0.0f;
        if (g < n8) {
            const float4 a = reinterpret_cast<const float4*>(tab)[2 * g];
            const float4 b = reinterpret_cast<const float4*>(tab)[2 * g + 1];
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t w[2] = {0, 0};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int X = __float2int_rn(v[i] * inv);
                X = X > 127 ? 127 : (X < -127 ? -127 : X);
                const float r = __fmaf_rn(-s, (float)X, v[i]);
                rs = __fmaf_rn(r, r, rs);
                w[i >> 2] |= (uint32_t)(X & 0xff) << (8 * (i & 3));
            }
            reinterpret_cast<uint2*>(out8)[g] = make_uint2(w[0], w[1]);
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) rs += __shfl_xor(rs, off, 64);
        mx = fmaxf(mx, rs);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) smax[w] = mx;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(reinterpret_cast<uint32_t*>(out_resid), __float_as_uint(fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]))));
}

// Table preparation for the screen, one coalesced pass: the bf16 shadow of the rows (RNE, what
// v_cvt_pk_bf16_f32 gives) and the statistics the error bound needs — max row L2 norm (upper bound) and
// finiteness.  A thread converts 8 consecutive values; DIM/8 neighbouring lanes share a row.
template <int DIM>
__global__ __launch_bounds__(256) void table_shadow_kernel(const float* __restrict__ tab, uint64_t rows,
                                                           uint16_t* __restrict__ out16,
                                                           float* __restrict__ out_max,
                                                           uint32_t* __restrict__ out_nonfinite,
                                                           float* __restrict__ out_blk_norm2) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    constexpr int G = DIM / 8;                       // lanes per row (8 or 16)
    __shared__ float smax[4];
    __shared__ uint32_t sbad[4];
    const uint64_t n8 = rows * (uint64_t)G;          // 8-value groups in the table
    float mx = 0.0f;
    uint32_t bad = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ((n8 + 63) & ~63ull);
         g += (uint64_t)gridDim.x * blockDim.x) {
        float ss = 0.0f;
        if (g < n8) {
            const float4 a = reinterpret_cast<const float4*>(tab)[2 * g];
            const float4 b = reinterpret_cast<const float4*>(tab)[2 * g + 1];
            const f32x2 p0 = {a.x, a.y}, p1 = {a.z, a.w}, p2 = {b.x, b.y}, p3 = {b.z, b.w};
            uint4 o;
            o.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(p0, bf16x2));
            o.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(p1, bf16x2));
            o.z = __builtin_bit_cast(uint32_t, __builtin_convertvector(p2, bf16x2));
            o.w = __builtin_bit_cast(uint32_t, __builtin_convertvector(p3, bf16x2));
            reinterpret_cast<uint4*>(out16)[g] = o;
            ss = a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w + b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) ss += __shfl_xor(ss, off, 64);     // the row's sum of squares
        if (!(ss < 3.0e38f)) bad = 1;                 // NaN, inf or overflow
        mx = fmaxf(mx, ss);
        // largest row norm^2 of the 32-row block: a wave holds 64 / G consecutive rows of one block
        float wm = ss;
#pragma unroll
        for (int off = G; off < 64; off <<= 1) wm = fmaxf(wm, __shfl_xor(wm, off, 64));
        if ((threadIdx.x & 63) == 0 && g < n8)
            atomicMax(reinterpret_cast<uint32_t*>(out_blk_norm2) + (g / G) / kPieceRows, __float_as_uint(fmaxf(wm, 0.0f)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        bad |= (uint32_t)__shfl_xor((int)bad, off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smax[w] = mx; sbad[w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
        atomicMax(reinterpret_cast<uint32_t*>(out_max), __float_as_uint(m));   // non-negative floats order as uints
        if (sbad[0] | sbad[1] | sbad[2] | sbad[3]) atomicOr(out_nonfinite, 1u);
    }
}

// squared-Euclidean recall: |x|^2 of every row as a k-ascending fmaf chain (the specification's)
__global__ void row_norm2_kernel(const float* __restrict__ tab, uint64_t rows, uint32_t dim, float* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float4* x = reinterpret_cast<const float4*>(tab + r * dim);
    float s = 0.0f;
    for (uint32_t c = 0; c < dim / 4; ++c) {
        const float4 v = x[c];
        s = __fmaf_rn(v.x, v.x, s);
        s = __fmaf_rn(v.y, v.y, s);
        s = __fmaf_rn(v.z, v.z, s);
        s = __fmaf_rn(v.w, v.w, s);
    }
    out[r] = s;
}

// ---------------------------------------------------------------------------------------------
// Threshold predictor.  A query's scores over the table are a projection of the rows: mean mu.q, variance q'Sq, and —
// 128 terms each — close to Gaussian, so the K-th best of N rows sits z standard deviations above the mean, with z
// nearly the same for every query of a workload.  mu and S come from a row sample (with the table's statistics); z is
// not assumed but OBSERVED: every verified batch reports (K-th best − mu.q) / sigma_q of its queries.  Once the
// observed z is tight, the first thresholds of a batch are mu.q + (mean z − margin) sigma_q: the pilot sample — two
// small scan launches, a re-scoring and two selects, 0.35 ms that nothing overlaps — is skipped.  Exactness does
// not depend on any of this: a threshold that turns out too high leaves a query short of K candidates, which the
// plan check sees, and the batch re-runs on the pilot plan (and the table stays on it for a while).
// ---------------------------------------------------------------------------------------------
// second moments of a row sample: workgroup b walks sample rows b, b + G, ...; thread (ty, tx) of a 16 x 16 grid owns
// the 8 x 8 patch (i = ty + 16a, j = tx + 16b) of sum x_i x_j; 16 rows are staged per barrier pair
__global__ __launch_bounds__(256) void pred_moments_kernel(const float* __restrict__ tab, uint64_t rows, uint64_t stride,
                                                           uint64_t n_sample, float* __restrict__ sum1, float* __restrict__ sum2) {
    __shared__ float xs[16][128 + 4];
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.0f;
    float s1 = 0.0f;                                       // thread t < 128: sum of column t
    for (uint64_t r0 = (uint64_t)blockIdx.x * 16; r0 < n_sample; r0 += (uint64_t)gridDim.x * 16) {
        __syncthreads();
        for (uint32_t e = tid; e < 16 * 32; e += 256) {    // 16 rows x 32 quads
            const uint32_t rr = e >> 5, qd = e & 31;
            const uint64_t sr = r0 + rr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sr < n_sample) {
                const uint64_t row = sr * stride < rows ? sr * stride : rows - 1;
                v = *reinterpret_cast<const float4*>(tab + row * 128 + 4 * qd);
            }
            *reinterpret_cast<float4*>(&xs[rr][4 * qd]) = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < 16; ++rr) {
            float xi[8], xj[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                xi[a] = xs[rr][ty + 16 * a];
                xj[a] = xs[rr][tx + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = __fmaf_rn(xi[a], xj[b], acc[a][b]);
            if (tid < 128) s1 += xs[rr][tid];
        }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) atomicAdd(&sum2[(ty + 16 * a) * 128 + tx + 16 * b], acc[a][b]);
    if (tid < 128) atomicAdd(&sum1[tid], s1);
}
// sums → mean and covariance in place; the observation block behind them is cleared
__global__ void pred_finish_kernel(float* __restrict__ pred, uint64_t n_sample) {
    const uint32_t i = blockIdx.x, j = threadIdx.x;        // 128 x 128
    const float inv = 1.0f / (float)n_sample;
    const float mi = pred[i] * inv, mj = pred[j] * inv;
    const float c = pred[128 + i * 128 + j] * inv - mi * mj;
    pred[128 + i * 128 + j] = c;                           // (the raw column sums pred[0..127] are turned into means by the next launch)
}
__global__ void pred_means_kernel(float* __restrict__ pred, uint64_t n_sample) {
    const uint32_t j = threadIdx.x;
    if (j < 128) pred[j] = pred[j] / (float)n_sample;
    if (j < 8) reinterpret_cast<uint32_t*>(pred + 128 + 128 * 128)[j] = 0u;          // n, sum z, sum z^2, min z (doubles)
    if (j == 0) reinterpret_cast<double*>(pred + 128 + 128 * 128)[3] = 1e300;
}

// statistics + shadow of a table (lazily, cached until the next upload / fill): int8 for dim 128 (two passes:
// statistics, then quantisation with the table's scale), bf16 for dim 64.
// Tables the screen cannot serve (other dims, no memory for the shadow) keep stats_valid = false.
std::mutex g_table_state_mu;   // table_state.hpp: guards pg_table::derived and pg_table::learned of every table
int ensure_table_stats(pg_ctx* ctx, const pg_table* t) {
    std::lock_guard<std::mutex> state_guard(g_table_state_mu);
    if (t->derived.stats_valid || t->derived.shadow_failed) return PG_OK;
    t->derived.stats_rebuilt();                       // the 4-bit shadow, the residual shadow and the threshold model follow the rows too
    t->learned.stats_rebuilt();
    if (t->dim != 64 && t->dim != 128) { t->derived.shadow_failed = true; return PG_OK; }
    bool i8 = t->dim == 128;
    void* p;
    int rc;
    if ((rc = scratch_reserve(ctx, kSlotStatus, 4096, &p))) return rc;
    float* d_max = (float*)p + 300;                   // [300] max norm^2, [301] non-finite flag, [302] max |x|, [303] max residual^2, [304] sum of norm^2
    uint32_t* d_bad = (uint32_t*)p + 301;
    PG_HIP(hipMemsetAsync(d_max, 0, 20, ctx->stream));
    const uint32_t grid = (uint32_t)ctx->num_cus * 16;
    if (i8) {
        // statistics first: they decide between the two shadows
        table_stats_kernel<128><<<grid, 256, 0, ctx->stream>>>(t->d, t->rows, d_max, d_bad, d_max + 2, d_max + 4);
        PG_HIP(hipGetLastError());
        PG_HIP(hipMemcpyAsync(ctx->h_status + 300, d_max, 20, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        float mx, amx, sumsq;
        memcpy(&mx, ctx->h_status + 300, 4);
        memcpy(&amx, ctx->h_status + 302, 4);
        memcpy(&sumsq, ctx->h_status + 304, 4);
        t->derived.all_finite = ctx->h_status[301] == 0;
        t->derived.max_norm = sqrtf(mx) * 1.0001f;
        t->derived.s8 = fmaxf(amx / 127.0f, 1e-30f);
        t->derived.resid8 = 0.0f;
        // One scale for the table only works when the largest element is not far above the typical row: the int8
        // margin is ~ s8 sqrt(dim / 12) per unit of ||q|| for EVERY row, the bf16 margin 0.008 x the row's own norm.
        // Heavy tails or outliers (a Student-t table: int8 margin 130 x the bf16 one, every row a suspect, 560 ms per
        // recall instead of 2.4) go to the bf16 shadow with per-block norms.
        const float rms_norm = sqrtf(sumsq / (float)(t->rows ? t->rows : 1));
        if (t->derived.all_finite && t->derived.s8 * sqrtf((float)t->dim / 12.0f) > 4.0f * kScreenEps * rms_norm) i8 = false;
    }
    if (i8) {
        if (!t->derived.d8) {
            const size_t bytes = (t->rows + 64) * (size_t)t->dim;
            if (hipMalloc((void**)&t->derived.d8, bytes) != hipSuccess) {
                (void)hipGetLastError();
                t->derived.d8 = nullptr;
                t->derived.shadow_failed = true;              // stay on the exact scan
                return PG_OK;
            }
            PG_HIP(hipMemsetAsync(t->derived.d8 + t->rows * (size_t)t->dim, 0, 64 * (size_t)t->dim, ctx->stream));
        }
        if (t->derived.all_finite) {
            table_quant8_kernel<128><<<grid, 256, 0, ctx->stream>>>(t->d, t->rows, t->derived.s8, t->derived.d8, d_max + 3);
            PG_HIP(hipGetLastError());
            PG_HIP(hipMemcpyAsync(ctx->h_status + 303, d_max + 3, 4, hipMemcpyDeviceToHost, ctx->stream));
            PG_HIP(hipStreamSynchronize(ctx->stream));
            float r2;
            memcpy(&r2, ctx->h_status + 303, 4);
            // (the residuals were accumulated in fp32: a relative 1e-3 and an absolute 1e-6 N cover that)
            t->derived.resid8 = sqrtf(r2) * 1.001f + 1e-6f * t->derived.max_norm;
        }
        t->derived.shadow_is_i8 = true;
        t->derived.stats_valid = true;
        return PG_OK;
    }
    const size_t n_blk = (size_t)((t->rows + kPieceRows - 1) / kPieceRows) + 2;
    if (!t->derived.d16) {
        const size_t bytes = (t->rows + 64) * (size_t)t->dim * 2;
        if (hipMalloc((void**)&t->derived.d16, bytes) != hipSuccess) {
            (void)hipGetLastError();
            t->derived.d16 = nullptr;
            t->derived.shadow_failed = true;                  // stay on the exact scan
            return PG_OK;
        }
        PG_HIP(hipMemsetAsync(t->derived.d16 + t->rows * (size_t)t->dim, 0, 64 * (size_t)t->dim * 2, ctx->stream));
    }
    if (!t->derived.dnorm2 && hipMalloc((void**)&t->derived.dnorm2, n_blk * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        t->derived.dnorm2 = nullptr;
        t->derived.shadow_failed = true;
        return PG_OK;
    }
    PG_HIP(hipMemsetAsync(t->derived.dnorm2, 0, n_blk * sizeof(float), ctx->stream));
    PG_HIP(hipMemsetAsync(d_max, 0, 8, ctx->stream));
    if (t->dim == 64) table_shadow_kernel<64><<<grid, 256, 0, ctx->stream>>>(t->d, t->rows, t->derived.d16, d_max, d_bad, t->derived.dnorm2);
    else table_shadow_kernel<128><<<grid, 256, 0, ctx->stream>>>(t->d, t->rows, t->derived.d16, d_max, d_bad, t->derived.dnorm2);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(ctx->h_status + 300, d_max, 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    float mx;
    memcpy(&mx, ctx->h_status + 300, 4);
    t->derived.all_finite = ctx->h_status[301] == 0;
    t->derived.max_norm = sqrtf(mx) * 1.0001f;
    t->derived.shadow_is_i8 = false;
    t->derived.stats_valid = true;
    return PG_OK;
}

// the threshold model's row sample: rows min(s * stride, rows - 1), s < n_sample
static inline void pred_sample(uint64_t rows, uint64_t* n_sample, uint64_t* stride) {
    *n_sample = rows < (1u << 20) ? rows : (1u << 20);
    *stride = rows / *n_sample;
}

// the threshold model of a table (dim 128): mean and covariance of a row sample, built once per generation of the rows
int ensure_pred_model(pg_ctx* ctx, const pg_table* t) {
    std::lock_guard<std::mutex> state_guard(g_table_state_mu);
    if (t->derived.pred_model) return PG_OK;
    const size_t bytes = (size_t)(128 + 128 * 128) * 4 + 5 * 8;   // mean | covariance (→ factor) | n, sum, sum2, min, total
    if (!t->derived.d_pred && hipMalloc((void**)&t->derived.d_pred, bytes) != hipSuccess) {
        (void)hipGetLastError();
        t->derived.d_pred = nullptr;
        return PG_OK;                                 // no model: the pilot plan serves
    }
    PG_HIP(hipMemsetAsync(t->derived.d_pred, 0, bytes, ctx->stream));
    uint64_t n_sample, stride;
    pred_sample(t->rows, &n_sample, &stride);
    pred_moments_kernel<<<(uint32_t)ctx->num_cus, 256, 0, ctx->stream>>>(t->d, t->rows, stride, n_sample, t->derived.d_pred, t->derived.d_pred + 128);
    pred_finish_kernel<<<128, 128, 0, ctx->stream>>>(t->derived.d_pred, n_sample);
    pred_means_kernel<<<1, 128, 0, ctx->stream>>>(t->derived.d_pred, n_sample);
    PG_HIP(hipGetLastError());
    PG_HIP(hipStreamSynchronize(ctx->stream));        // other contexts of the device use the model from their own streams
    t->derived.pred_model = true;
    t->learned.model_rebuilt();
    return PG_OK;
}

// |x|^2 of every row, for the squared-Euclidean recall (lazily, cached until the next upload / fill; shared by the contexts
// of a device like the shadows)
int ensure_table_nx(pg_ctx* ctx, const pg_table* t) {
    std::lock_guard<std::mutex> state_guard(g_table_state_mu);
    if (t->derived.nx_valid) return PG_OK;
    const uint32_t nblocks = (uint32_t)((t->rows + kPieceRows - 1) / kPieceRows);
    if (!t->derived.d_nx) PG_HIP(hipMalloc((void**)&t->derived.d_nx, (t->rows + 64) * sizeof(float)));
    if (!t->derived.d_nxmin) PG_HIP(hipMalloc((void**)&t->derived.d_nxmin, ((size_t)nblocks + 64) * sizeof(float)));
    PG_HIP(hipMemsetAsync(t->derived.d_nx + t->rows, 0, 64 * sizeof(float), ctx->stream));
    PG_HIP(hipMemsetAsync(t->derived.d_nxmin + nblocks, 0, 64 * sizeof(float), ctx->stream));
    row_norm2_kernel<<<(uint32_t)((t->rows + 255) / 256), 256, 0, ctx->stream>>>(t->d, t->rows, t->dim, t->derived.d_nx);
    void* p;
    int rc;
    if ((rc = scratch_reserve(ctx, kSlotStatus, 4096, &p))) return rc;
    double* d_st = reinterpret_cast<double*>((char*)p + 2048);
    PG_HIP(hipMemsetAsync(d_st, 0, 16, ctx->stream));
    block_nxmin_kernel<<<(nblocks + 255) / 256, 256, 0, ctx->stream>>>(t->derived.d_nx, t->rows, t->derived.d_nxmin, nblocks, d_st);
    PG_HIP(hipGetLastError());
    double h_st[2] = {0.0, 0.0};
    PG_HIP(hipMemcpyAsync(h_st, d_st, 16, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    // What the per-block cutoff gives away: a row's cutoff sits (|x|^2 - min of its block) / 2 below its own, in inner-product
    // units whose spread over the table is about |x| |q| / sqrt(dim) ~ mean|x|^2 / sqrt(dim) for queries like the rows.  Normalised
    // rows: 0.  N(0, 1) rows: 1.5 spreads — then nearly every block holds suspects and the exact scan is the faster pass.
    const double mean_nx = t->rows ? h_st[1] / (double)t->rows : 0.0;
    t->derived.l2_slack = mean_nx > 0.0 ? (float)((h_st[0] / (double)t->rows) * 0.5 / (mean_nx / sqrt((double)t->dim))) : 0.0f;
    if (ctx->knobs.debug_scan) fprintf(stderr, "[pg] squared-Euclidean recall: per-block cutoff slack %.3f score spreads\n", t->derived.l2_slack);
    t->derived.nx_valid = true;
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_table_screen_info(pg_ctx* ctx, const pg_table* t, int* out_elem_bytes, float* out_scale, float* out_resid) {
    PG_REQUIRE(ctx && t, "pg_table_screen_info: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    int rc;
    if ((rc = pg::ensure_table_stats(ctx, t))) return rc;
    const bool screened = t->derived.stats_valid && t->derived.all_finite;
    if (out_elem_bytes) *out_elem_bytes = screened ? (t->derived.shadow_is_i8 ? 1 : 2) : 0;
    if (out_scale) *out_scale = screened && t->derived.shadow_is_i8 ? t->derived.s8 : 0.0f;
    if (out_resid) *out_resid = screened && t->derived.shadow_is_i8 ? t->derived.resid8 : 0.0f;
    return PG_OK;
}

// Diagnostics of a table's derived state.  Lock order as table_state.hpp prescribes for a reader of `derived`: ctx->mu, the
// table's shared lock, then (inside the ensure_* calls) g_table_state_mu; what is read afterwards was built by those calls.
int pg_table_derived_info(pg_ctx* ctx, const pg_table* t, uint32_t parts, pg_table_derived_t* out) {
    PG_REQUIRE(ctx && t && out, "pg_table_derived_info: NULL argument");
    const uint32_t known = PG_DERIVED_STATS | PG_DERIVED_I4 | PG_DERIVED_R2 | PG_DERIVED_NX | PG_DERIVED_PRED;
    PG_REQUIRE((parts & ~known) == 0, "pg_table_derived_info: unknown parts 0x%x", parts);
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    int rc;
    if ((rc = pg::ensure_table_stats(ctx, t))) return rc;     // always first: it is what resets the parts below after a write
    const pg::TableDerived& d = t->derived;
    const bool screened = d.stats_valid && d.all_finite;
    if ((parts & PG_DERIVED_I4) && (rc = pg::ensure_table_i4(ctx, t))) return rc;
    if ((parts & PG_DERIVED_R2) && (rc = pg::ensure_table_r2(ctx, t))) return rc;
    if ((parts & PG_DERIVED_NX) && (t->dim == 64 || t->dim == 128) && (rc = pg::ensure_table_nx(ctx, t))) return rc;
    // (the recall builds the model for int8-screened dim-128 tables only: the kernels assume 128 columns)
    if ((parts & PG_DERIVED_PRED) && t->dim == 128 && screened && d.shadow_is_i8 && (rc = pg::ensure_pred_model(ctx, t))) return rc;
    memset(out, 0, sizeof(*out));
    out->elem_bytes = screened ? (d.shadow_is_i8 ? 1 : 2) : 0;
    out->all_finite = d.stats_valid && d.all_finite ? 1 : 0;
    out->max_norm = d.stats_valid ? d.max_norm : 0.0f;
    out->s8 = screened && d.shadow_is_i8 ? d.s8 : 0.0f;
    out->resid8 = screened && d.shadow_is_i8 ? d.resid8 : 0.0f;
    out->i4_ok = d.i4_ok ? 1 : 0;
    if (d.i4_ok) { out->rho4 = d.rho4; out->rmax4 = d.rmax4; out->lam4 = d.lam4; }
    out->r2_ok = d.r2_ok ? 1 : 0;
    if (d.r2_ok) { out->s8r = d.s8r; out->resid2 = d.resid2; }
    out->nx_valid = d.nx_valid ? 1 : 0;
    if (d.nx_valid) out->l2_slack = d.l2_slack;
    out->pred_model = d.pred_model ? 1 : 0;
    if (d.pred_model) pg::pred_sample(t->rows, &out->pred_n_sample, &out->pred_stride);
    return PG_OK;
}

int pg_table_derived_read(pg_ctx* ctx, const pg_table* t, int which, uint64_t first, uint64_t n, void* out) {
    PG_REQUIRE(ctx && t && (n == 0 || out), "pg_table_derived_read: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    const pg::TableDerived& d = t->derived;
    const void* src = nullptr;
    uint64_t len = 0, esz = 0;
    bool built = false;
    {
        // a write since the last build invalidates everything (ensure_table_stats has not yet reset the later parts' flags)
        std::lock_guard<std::mutex> sg(pg::g_table_state_mu);
        const bool cur = d.stats_valid, screened = cur && d.all_finite;
        const uint64_t padded = t->rows + 64, nblk = (t->rows + pg::kPieceRows - 1) / pg::kPieceRows;
        switch (which) {
            case PG_DERIVED_ARR_I8: src = d.d8; len = padded * t->dim; esz = 1; built = screened && d.shadow_is_i8; break;
            case PG_DERIVED_ARR_BF16: src = d.d16; len = padded * t->dim; esz = 2; built = screened && !d.shadow_is_i8; break;
            case PG_DERIVED_ARR_BLKNORM2: src = d.dnorm2; len = nblk; esz = 4; built = screened && !d.shadow_is_i8; break;
            case PG_DERIVED_ARR_I4: src = d.d4; len = padded * 16; esz = 4; built = cur && d.i4_ok; break;
            case PG_DERIVED_ARR_I4S: src = d.d4s; len = padded; esz = 4; built = cur && d.i4_ok; break;
            case PG_DERIVED_ARR_I8R: src = d.d8r; len = padded * 128; esz = 1; built = cur && d.r2_ok; break;
            case PG_DERIVED_ARR_NX: src = d.d_nx; len = padded; esz = 4; built = d.nx_valid; break;
            case PG_DERIVED_ARR_NXMIN: src = d.d_nxmin; len = nblk; esz = 4; built = d.nx_valid; break;
            case PG_DERIVED_ARR_PRED: src = d.d_pred; len = 128 + 128 * 128 + 10; esz = 4; built = cur && d.pred_model; break;
            default: break;
        }
    }
    PG_REQUIRE(esz != 0, "pg_table_derived_read: unknown array %d", which);
    PG_REQUIRE(built && src, "pg_table_derived_read: array %d is not built (pg_table_derived_info builds it)", which);
    PG_REQUIRE(first <= len && n <= len - first, "pg_table_derived_read: elements [%llu,+%llu) outside array %d of %llu",
               (unsigned long long)first, (unsigned long long)n, which, (unsigned long long)len);
    if (n == 0) return PG_OK;
    PG_HIP(hipMemcpyAsync(out, (const char*)src + first * esz, n * esz, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

}  // extern "C"
