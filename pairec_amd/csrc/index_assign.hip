// index_assign.hip — the nearest-centroid assignment of pg_index_refresh's full path on the bf16 matrix pipe.
//
// The rule (index.hip: assign_kernel) gives row x the list of smallest d_L = fl(cn2[L] - 2 a_L), a_L the k-ascending fp32 fmaf
// chain of x.c_L, ties to the lower list.  Rows x lists x dim is 1 PFLOP at 100 M x 40 000 x 128 and the fp32 MFMA runs at the
// vector rate, so the matrix pipe is used as everywhere else in this library: as a rigorous screen whose survivors are
// confirmed with the rule's own chain.
//
//   screen   x and c are split into bf16 pairs (x = xh + xl + xr, |xr| <= 2^-18 |x|).  v_mfma_f32_32x32x16_bf16 accumulates
//            ch.xh into one fp32 tile and cl.xh + ch.xl into a second one (the cross terms are 2^-8 of the first: kept apart, their
//            2 dim additions round at that scale); s_L = fl(cn2[L] - 2 fl(hh + cross)).  The centroids are the A operand, the
//            rows the B operand: a lane holds 16 of a tile's 32 lists for ONE row (its partner lane l ^ 32 the other 16), so
//            the argmin epilogue needs no cross-lane traffic beyond one exchange of the running bound per tile.
//   bound    |s_L - d_L| <= e(x, L) = A ||x|| ||c_L|| + B cn2[L] + eta  (screen_bound_consts; derived in DESIGN.md 4.1i from the
//            split's truncation, the MFMA's fp32 accumulation, the chain's own rounding and the two final subtractions), proven for
//            rows and centroids with 2^-40 <= ||.||^2 <= 2^48 and finite elements.
//   discard  ub = the smallest s_M + e(x, M) seen so far.  A list with s_L - e(x, L) > ub cannot be the rule's argmin (nor tie with
//            it); the others are survivors, kept in four slots per lane (eight per row).
//   confirm  the survivors' d_L by the rule's chain from the fp32 rows and centroids, the rule's tie-break.  A row that ran out
//            of slots, or lies outside the range, is appended to the `wide` list: the caller runs assign_kernel over those rows.
//
// One workgroup of eight waves takes 512 rows at dim 64 (two 32-row B blocks per wave) or 256 at dim 128 (one), whose bf16
// fragments stay in registers for the whole sweep (64 of them), past all centroid tiles: a tile of 32 centroids (hi and lo, 16-B slots XOR-swizzled by centroid) is read
// from the split copy in L2 into registers while the previous one is multiplied, then stored into the other LDS buffer: one
// barrier per tile.
#include "common.hpp"
#include "rank_mlp.hpp"

namespace pg {
namespace {

constexpr int kAsWaves = 8;
constexpr int as_nb(int dim) { return 128 / dim; }                    // 32-row B blocks per wave: 64 fragment registers either way
constexpr int as_rows(int dim) { return kAsWaves * as_nb(dim) * 32; } // rows per workgroup
constexpr int kAsSlots = 4;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr float kRangeLo = 0x1p-40f, kRangeHi = 0x1p48f;      // the range of ||.||^2 the bound is proven for

// e(x, L) = A ||x|| ||c_L|| + B cn2[L] + eta, ||x|| and ||c_L|| upper bounds.  u = 2^-24.
//   |a~ - a| <= E ||x|| ||c||,  E = gamma_dim (the chain) + 1.01 gamma_(dim+2) (hi.hi tile and the final sum)
//                                  + 2^-7 gamma_(2 dim) (cross tile) + 3.02 x 2^-18 (the split's truncation)
//   |s - d|  <= 2 |a~ - a| + 2 u cn2 + 4.04 u ||x|| ||c||;  (1 + 2^-10) covers the fp32 evaluation of e itself
struct ScreenConsts { float A, B, eta; };
__host__ __device__ inline ScreenConsts screen_bound_consts(uint32_t dim) {
    const double u = 0x1p-24, d = (double)dim;
    auto gam = [&](double n) { return n * u / (1.0 - n * u); };
    const double E = gam(d) + 1.01 * gam(d + 2.0) + 0x1p-7 * gam(2.0 * d) + 3.02 * 0x1p-18;
    ScreenConsts c;
    c.A = (float)((2.0 * E + 4.04 * u) * (1.0 + 0x1p-10));
    c.B = (float)(2.0 * u * (1.0 + 0x1p-10));
    c.eta = 0x1p-90f;
    return c;
}

__device__ __forceinline__ float round_up_f(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, __builtin_inff());
    return f;
}

// the centroids' side of the screen, one thread per (padded) list: the bf16 hi / lo copies [nl_pad][dim], and meta[0] = cn2 (the
// rule's chain, as cnorm2_kernel), meta[1] >= ||c_L|| (fp64, rounded up), meta[2] = B cn2 + eta.  A padding list never wins
// (cn2 = +inf, operands 0).  *range |= 1 for a centroid outside the bound's range.
__global__ void screen_prep_kernel(const float* __restrict__ C, uint32_t nl, uint32_t nl_pad, uint32_t dim, uint16_t* __restrict__ hi,
                                   uint16_t* __restrict__ lo, float* __restrict__ meta, uint32_t* __restrict__ range) {
    const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= nl_pad) return;
    const ScreenConsts k = screen_bound_consts(dim);
    float s = 0.0f;
    double s64 = 0.0;
    bool bad = false;
    for (uint32_t c = 0; c < dim; c += 2) {
        float v0 = 0.0f, v1 = 0.0f;
        if (L < nl) { v0 = C[(size_t)L * dim + c]; v1 = C[(size_t)L * dim + c + 1]; }
        bad |= !isfinite(v0) || !isfinite(v1);
        s = __fmaf_rn(v0, v0, s);
        s = __fmaf_rn(v1, v1, s);
        s64 = fma((double)v0, (double)v0, s64);
        s64 = fma((double)v1, (double)v1, s64);
        uint32_t ph, pl;
        split_bf16x2(v0, v1, ph, pl);
        *reinterpret_cast<uint32_t*>(hi + (size_t)L * dim + c) = ph;
        *reinterpret_cast<uint32_t*>(lo + (size_t)L * dim + c) = pl;
    }
    if (L < nl) {
        meta[L] = s;
        meta[nl_pad + L] = round_up_f(sqrt(s64) * (1.0 + 0x1p-40));
        meta[2 * (size_t)nl_pad + L] = __fmaf_rn(k.B, s, k.eta);
        if (bad || !(s >= kRangeLo && s <= kRangeHi)) atomicOr(range, 1u);
    } else {
        meta[L] = __builtin_inff();
        meta[nl_pad + L] = 0.0f;
        meta[2 * (size_t)nl_pad + L] = 0.0f;
    }
}

// the slot of 16-B chunk q of centroid r's row in a tile (DIM x 2 bytes per row): XOR-swizzled so that the lanes of a
// ds_read_b128 group (different r, one q) fall on different bank slots
template <int DIM>
__device__ __forceinline__ int tile_off(int r, int q) {
    constexpr int SLOTS = DIM / 8;
    const int sw = DIM == 128 ? (r & 15) : ((r >> 1) & 7);
    return r * (DIM * 2) + ((q ^ sw) & (SLOTS - 1)) * 16;
}


// ---- the screen's arithmetic, shared by the assignment and by pg_index_screen_probe (which exposes it to the tests) ----------
// row `row`'s half h of the B fragments (k = 16 s + 8 h + j), its share of the fp32 chain of ||x||^2, whether an element is
// not finite; a row past n reads as zeros
template <int DIM>
__device__ __forceinline__ void screen_row_load(const float* __restrict__ X, uint64_t row, uint64_t n, int h, uint4 (&xh)[DIM / 16],
                                                uint4 (&xl)[DIM / 16], float& s2, bool& bad) {
#pragma unroll
    for (int s = 0; s < DIM / 16; ++s) {
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (row < n) {
            const float4* src = reinterpret_cast<const float4*>(X + row * DIM + 16 * s + 8 * h);
            v0 = src[0];
            v1 = src[1];
        }
        bad |= !isfinite(v0.x) || !isfinite(v0.y) || !isfinite(v0.z) || !isfinite(v0.w) || !isfinite(v1.x) || !isfinite(v1.y) ||
               !isfinite(v1.z) || !isfinite(v1.w);
        s2 = __fmaf_rn(v0.x, v0.x, s2); s2 = __fmaf_rn(v0.y, v0.y, s2); s2 = __fmaf_rn(v0.z, v0.z, s2); s2 = __fmaf_rn(v0.w, v0.w, s2);
        s2 = __fmaf_rn(v1.x, v1.x, s2); s2 = __fmaf_rn(v1.y, v1.y, s2); s2 = __fmaf_rn(v1.z, v1.z, s2); s2 = __fmaf_rn(v1.w, v1.w, s2);
        split_bf16x2(v0.x, v0.y, xh[s].x, xl[s].x);
        split_bf16x2(v0.z, v0.w, xh[s].y, xl[s].y);
        split_bf16x2(v1.x, v1.y, xh[s].z, xl[s].z);
        split_bf16x2(v1.z, v1.w, xh[s].w, xl[s].w);
    }
}
__device__ __forceinline__ bool screen_in_range(float n2) { return n2 >= kRangeLo && n2 <= kRangeHi; }
// A x (an upper bound of ||x||) from the fp32 chain of ||x||^2
__device__ __forceinline__ float screen_anx(float A, float s2) { return A * (sqrtf(s2) * (1.0f + 0x1p-10f)); }
// one tile (hi at tile, lo at tile + 32 DIM 2 bytes; tile_off's layout) against NB row blocks: hh += ch.xh, cr += cl.xh + ch.xl
template <int DIM, int NB>
__device__ __forceinline__ void screen_tile_mfma(const char* tile, int r, int h, const uint4 (&xh)[NB][DIM / 16],
                                                 const uint4 (&xl)[NB][DIM / 16], f32x16 (&hh)[NB], f32x16 (&cr)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) { hh[b][i] = 0.0f; cr[b][i] = 0.0f; }
#pragma unroll
    for (int s = 0; s < DIM / 16; ++s) {
        const int o = tile_off<DIM>(r, 2 * s + h);
        const bf16x8 ch = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(tile + o));
        const bf16x8 cl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(tile + 32 * DIM * 2 + o));
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, xh[b][s]), bl = __builtin_bit_cast(bf16x8, xl[b][s]);
            hh[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch, bh, hh[b], 0, 0, 0);
            cr[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl, bh, cr[b], 0, 0, 0);
            cr[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch, bl, cr[b], 0, 0, 0);
        }
    }
}
__device__ __forceinline__ float screen_s(float cn2, float hh, float cr) { return cn2 - 2.0f * (hh + cr); }
__device__ __forceinline__ float screen_e(float anx, float cn, float eb) { return __fmaf_rn(anx, cn, eb); }

template <int DIM>
__global__ __launch_bounds__(kAsWaves * 64) void assign_screen_kernel(const float* __restrict__ X, uint64_t n, const float* __restrict__ C,
                                                                      const uint16_t* __restrict__ chi, const uint16_t* __restrict__ clo,
                                                                      const float* __restrict__ meta, uint32_t nl, uint32_t nl_pad,
                                                                      uint32_t* __restrict__ out, uint32_t* __restrict__ wide,
                                                                      uint32_t* __restrict__ wide_n, uint32_t* __restrict__ flag) {
    constexpr int KS = DIM / 16, SLOTS = DIM / 8, NB = as_nb(DIM), kAsRows = as_rows(DIM);
    constexpr int TILE_B = 32 * DIM * 2;                      // one of hi / lo
    constexpr int CHUNKS = 2 * 32 * SLOTS / (kAsWaves * 64);  // 16-B chunks of a tile (hi + lo) per thread
    static_assert(CHUNKS >= 1 && 2 * 32 * SLOTS % (kAsWaves * 64) == 0, "tile chunks");
    __shared__ __attribute__((aligned(16))) char tiles[2][2 * TILE_B];
    __shared__ __attribute__((aligned(16))) float metas[2][3][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const uint64_t row0 = (uint64_t)blockIdx.x * kAsRows + (uint64_t)wave * (NB * 32);
    const ScreenConsts kc = screen_bound_consts(DIM);

    // ---- the wave's rows: bf16 hi / lo B fragments (lane: row r of block b, k = 16 s + 8 h + j), the row's norm and range
    uint4 xh[NB][KS], xl[NB][KS];
    float anx[NB];                       // A x (an upper bound of ||x||)
    bool inrange[NB];
    bool bad = false;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint64_t row = row0 + 32 * b + r;
        float s2 = 0.0f;
        screen_row_load<DIM>(X, row, n, h, xh[b], xl[b], s2, bad);
        s2 += __shfl_xor(s2, 32);        // (the two halves of the row; a non-finite or overflowing square leaves the range)
        inrange[b] = screen_in_range(s2);
        anx[b] = screen_anx(kc.A, s2);
    }
    if (bad) atomicOr(flag, 1u);

    // ---- the sweep over the centroid tiles
    const uint32_t nt = nl_pad / 32;
    static_assert(CHUNKS <= 2, "tile chunks");
    uint4 pre0 = make_uint4(0, 0, 0, 0), pre1 = pre0;
    float pre_m = 0.0f;
    // chunk e of a tile: part (hi / lo), centroid rr, 16-B chunk q of its row
    const int e0 = tid, e1 = tid + kAsWaves * 64;
    const int src0 = ((e0 / SLOTS) % 32) * DIM + (e0 % SLOTS) * 8, src1 = ((e1 / SLOTS) % 32) * DIM + (e1 % SLOTS) * 8;
    const int dst0 = (e0 / (32 * SLOTS)) * TILE_B + tile_off<DIM>((e0 / SLOTS) % 32, e0 % SLOTS);
    const int dst1 = (e1 / (32 * SLOTS)) * TILE_B + tile_off<DIM>((e1 / SLOTS) % 32, e1 % SLOTS);
    const uint16_t* const g0 = (e0 / (32 * SLOTS) ? clo : chi) + src0;
    const uint16_t* const g1 = (e1 / (32 * SLOTS) ? clo : chi) + src1;
    auto fetch = [&](uint32_t t) {
        pre0 = *reinterpret_cast<const uint4*>(g0 + (size_t)t * 32 * DIM);
        if constexpr (CHUNKS > 1) pre1 = *reinterpret_cast<const uint4*>(g1 + (size_t)t * 32 * DIM);
        if (tid < 96) pre_m = meta[(size_t)(tid >> 5) * nl_pad + (size_t)t * 32 + (tid & 31)];
    };
    auto stash = [&](int buf) {
        *reinterpret_cast<uint4*>(&tiles[buf][dst0]) = pre0;
        if constexpr (CHUNKS > 1) *reinterpret_cast<uint4*>(&tiles[buf][dst1]) = pre1;
        if (tid < 96) metas[buf][tid >> 5][tid & 31] = pre_m;
    };
    float ub[NB], slo[NB][kAsSlots];
    uint32_t sid[NB][kAsSlots];
    bool over[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        ub[b] = __builtin_inff();
        over[b] = false;
#pragma unroll
        for (int j = 0; j < kAsSlots; ++j) { slo[b][j] = __builtin_inff(); sid[b][j] = kNone; }
    }
    fetch(0);
    stash(0);
    __syncthreads();
    for (uint32_t t = 0; t < nt; ++t) {
        const int buf = (int)(t & 1);
        if (t + 1 < nt) fetch(t + 1);
        f32x16 hh[NB], cr[NB];
        screen_tile_mfma<DIM, NB>(tiles[buf], r, h, xh, xl, hh, cr);
        // the argmin epilogue: register 4 g + i of a lane is list 8 g + 4 h + i of the tile, for the lane's row
        float4 m_cn2[4], m_cn[4], m_eb[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            m_cn2[g] = *reinterpret_cast<const float4*>(&metas[buf][0][8 * g + 4 * h]);
            m_cn[g] = *reinterpret_cast<const float4*>(&metas[buf][1][8 * g + 4 * h]);
            m_eb[g] = *reinterpret_cast<const float4*>(&metas[buf][2][8 * g + 4 * h]);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float sv[16], ev[16];
            float tmin = __builtin_inff();
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int g = i >> 2, c = i & 3;
                const float cn2 = c == 0 ? m_cn2[g].x : c == 1 ? m_cn2[g].y : c == 2 ? m_cn2[g].z : m_cn2[g].w;
                const float cn = c == 0 ? m_cn[g].x : c == 1 ? m_cn[g].y : c == 2 ? m_cn[g].z : m_cn[g].w;
                const float eb = c == 0 ? m_eb[g].x : c == 1 ? m_eb[g].y : c == 2 ? m_eb[g].z : m_eb[g].w;
                sv[i] = screen_s(cn2, hh[b][i], cr[b][i]);
                ev[i] = screen_e(anx[b], cn, eb);
                tmin = fminf(tmin, sv[i] + ev[i]);
            }
            tmin = fminf(tmin, __shfl_xor(tmin, 32));
            ub[b] = fminf(ub[b], tmin);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float lo = sv[i] - ev[i];
                if (lo <= ub[b]) {
                    const uint32_t L = t * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                    bool placed = false;
#pragma unroll
                    for (int j = 0; j < kAsSlots; ++j) {
                        if (!placed && (sid[b][j] == kNone || slo[b][j] > ub[b])) {
                            slo[b][j] = lo;
                            sid[b][j] = L;
                            placed = true;
                        }
                    }
                    if (!placed) over[b] = true;
                }
            }
        }
        if (t + 1 < nt) stash(buf ^ 1);
        __syncthreads();
    }

    // ---- confirm: the rule's chain for the survivors, its tie-break; the partner lane holds the other half of the lists
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint64_t row = row0 + 32 * b + r;
        float best = __builtin_inff();
        uint32_t bi = kNone;
        if (row < n && inrange[b]) {
#pragma unroll
            for (int j = 0; j < kAsSlots; ++j) {
                const uint32_t L = sid[b][j];
                if (L >= nl || !(slo[b][j] <= ub[b])) continue;
                const float* x = X + row * DIM;
                const float* c = C + (size_t)L * DIM;
                float acc = 0.0f;
                for (int k = 0; k < DIM; k += 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + k), cv = *reinterpret_cast<const float4*>(c + k);
                    acc = __fmaf_rn(xv.x, cv.x, acc);
                    acc = __fmaf_rn(xv.y, cv.y, acc);
                    acc = __fmaf_rn(xv.z, cv.z, acc);
                    acc = __fmaf_rn(xv.w, cv.w, acc);
                }
                const float d = meta[L] - 2.0f * acc;
                if (d < best || (d == best && L < bi)) { best = d; bi = L; }
            }
        }
        const float ob = __shfl_xor(best, 32);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, 32);
        const bool oo = __shfl_xor((int)over[b], 32) != 0;
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        if (h == 0 && row < n) {
            if (!inrange[b] || over[b] || oo || bi >= nl) wide[atomicAdd(wide_n, 1u)] = (uint32_t)row;
            else out[row] = bi;
        }
    }
}

template <int DIM>
int screen_launch(pg_ctx* ctx, const float* X, uint64_t n, const float* C, const uint16_t* chi, const uint16_t* clo, const float* meta,
                  uint32_t nl, uint32_t nl_pad, uint32_t* out, uint32_t* wide, uint32_t* wide_n, uint32_t* flag) {
    assign_screen_kernel<DIM><<<(uint32_t)((n + as_rows(DIM) - 1) / as_rows(DIM)), kAsWaves * 64, 0, ctx->stream>>>(X, n, C, chi, clo, meta, nl, nl_pad,
                                                                                                           out, wide, wide_n, flag);
    PG_HIP(hipGetLastError());
    return PG_OK;
}


// pg_index_screen_probe: the screen's values and bounds themselves, one wave per 32 rows x 32 lists, through the same loads,
// MFMA sequence and formulas as the assignment: s[row][L], e[row][L] (+inf where the row or the centroid is outside the range
// the bound is claimed for)
template <int DIM>
__global__ __launch_bounds__(64) void screen_probe_kernel(const float* __restrict__ X, uint32_t n, const uint16_t* __restrict__ chi,
                                                          const uint16_t* __restrict__ clo, const float* __restrict__ meta, uint32_t nl,
                                                          uint32_t nl_pad, float* __restrict__ out_s, float* __restrict__ out_e) {
    constexpr int SLOTS = DIM / 8, TILE_B = 32 * DIM * 2;
    __shared__ __attribute__((aligned(16))) char tile[2 * TILE_B];
    __shared__ __attribute__((aligned(16))) float metas[3][32];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const uint32_t t = blockIdx.x;
    const uint64_t row = (uint64_t)blockIdx.y * 32 + r;
    const ScreenConsts kc = screen_bound_consts(DIM);
    uint4 xh[1][DIM / 16], xl[1][DIM / 16];
    float s2 = 0.0f;
    bool bad = false;
    screen_row_load<DIM>(X, row, n, h, xh[0], xl[0], s2, bad);
    s2 += __shfl_xor(s2, 32);
    for (int e = lane; e < 2 * 32 * SLOTS; e += 64) {
        const int part = e / (32 * SLOTS), rr = (e / SLOTS) % 32, q = e % SLOTS;
        *reinterpret_cast<uint4*>(&tile[part * TILE_B + tile_off<DIM>(rr, q)]) =
            *reinterpret_cast<const uint4*>((part ? clo : chi) + ((size_t)t * 32 + rr) * DIM + q * 8);
    }
    for (int e = lane; e < 96; e += 64) metas[e >> 5][e & 31] = meta[(size_t)(e >> 5) * nl_pad + (size_t)t * 32 + (e & 31)];
    __syncthreads();
    f32x16 hh[1], cr[1];
    screen_tile_mfma<DIM, 1>(tile, r, h, xh, xl, hh, cr);
    const float anx = screen_anx(kc.A, s2);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = 8 * (i >> 2) + 4 * h + (i & 3);
        const uint32_t L = t * 32 + c;
        if (row >= n || L >= nl) continue;
        const float cn2 = metas[0][c];
        const bool ok = screen_in_range(s2) && screen_in_range(cn2);
        out_s[row * nl + L] = screen_s(cn2, hh[0][i], cr[0][i]);
        out_e[row * nl + L] = ok ? screen_e(anx, metas[1][c], metas[2][c]) : __builtin_inff();
    }
}

uint32_t pad32(uint32_t nl) { return (nl + 31u) & ~31u; }

}  // namespace

// workspace: hi | lo [nl_pad][dim] bf16, meta [3][nl_pad], the range word
size_t assign_screen_ws_bytes(uint32_t nl, uint32_t dim) {
    const size_t np = pad32(nl);
    return 2 * np * dim * 2 + 3 * np * 4 + 256;
}

namespace {
struct ScreenWs { uint16_t *chi, *clo; float* meta; uint32_t* range; uint32_t np; };
ScreenWs screen_ws(void* ws, uint32_t nl, uint32_t dim) {
    ScreenWs w;
    w.np = pad32(nl);
    w.chi = (uint16_t*)ws;
    w.clo = w.chi + (size_t)w.np * dim;
    w.meta = (float*)(w.clo + (size_t)w.np * dim);
    w.range = (uint32_t*)(w.meta + 3 * (size_t)w.np);
    return w;
}
// the centroids' split copy and per-list constants into the workspace; *in_range: no centroid lies outside the bound's range
int screen_prep(pg_ctx* ctx, const ScreenWs& w, uint32_t dim, const float* C, uint32_t nl, bool* in_range) {
    hipStream_t s = ctx->stream;
    PG_HIP(hipMemsetAsync(w.range, 0, 4, s));
    screen_prep_kernel<<<(w.np + 63) / 64, 64, 0, s>>>(C, nl, w.np, dim, w.chi, w.clo, w.meta, w.range);
    PG_HIP(hipGetLastError());
    uint32_t h_range = 0;
    PG_HIP(hipMemcpyAsync(&h_range, w.range, 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    *in_range = h_range == 0;
    return PG_OK;
}
}  // namespace

int assign_screen_launch(pg_ctx* ctx, uint32_t dim, const float* X, uint64_t n, const float* C, uint32_t nl, void* ws, uint32_t* out,
                         uint32_t* wide, uint32_t* wide_n, uint32_t* flag) {
    if (dim != 64 && dim != 128) return PG_ERR_UNSUPPORTED;
    const ScreenWs w = screen_ws(ws, nl, dim);
    uint16_t* const chi = w.chi;
    uint16_t* const clo = w.clo;
    float* const meta = w.meta;
    const uint32_t np = w.np;
    bool in_range;
    int rc;
    if ((rc = screen_prep(ctx, w, dim, C, nl, &in_range))) return rc;
    if (!in_range) return PG_ERR_UNSUPPORTED;
    return dim == 64 ? screen_launch<64>(ctx, X, n, C, chi, clo, meta, nl, np, out, wide, wide_n, flag)
                     : screen_launch<128>(ctx, X, n, C, chi, clo, meta, nl, np, out, wide, wide_n, flag);
}

}  // namespace pg

extern "C" int pg_index_screen_probe(pg_ctx* ctx, uint32_t dim, const float* rows, uint32_t n, const float* centroids, uint32_t n_lists,
                                     float* out_s, float* out_e) {
    PG_REQUIRE(ctx && rows && centroids && out_s && out_e, "pg_index_screen_probe: NULL argument");
    PG_REQUIRE(dim == 64 || dim == 128, "pg_index_screen_probe: dim=%u (the screen serves 64 and 128)", dim);
    PG_REQUIRE(n >= 1 && n <= 65536 && n_lists >= 1 && n_lists <= 65536, "pg_index_screen_probe: 1 <= n, n_lists <= 65536");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t xb = (size_t)n * dim * 4, cb = (size_t)n_lists * dim * 4, ob = (size_t)n * n_lists * 4;
    const size_t wb = pg::assign_screen_ws_bytes(n_lists, dim);
    float *d_x, *d_c, *d_s, *d_e; void* ws; int rc;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& c) {
            d_x = c.take<float>((size_t)n * dim);
            d_c = c.take<float>((size_t)n_lists * dim);
            d_s = c.take<float>((size_t)n * n_lists);
            d_e = c.take<float>((size_t)n * n_lists);
            ws = c.bytes(wb);
        }))) return rc;
    const pg::ScreenWs w = pg::screen_ws(ws, n_lists, dim);
    PG_HIP(hipMemcpyAsync(d_x, rows, xb, hipMemcpyHostToDevice, s));
    PG_HIP(hipMemcpyAsync(d_c, centroids, cb, hipMemcpyHostToDevice, s));
    bool in_range;
    if ((rc = pg::screen_prep(ctx, w, dim, d_c, n_lists, &in_range))) return rc;
    const dim3 grid(w.np / 32, (n + 31) / 32);
    if (dim == 64) pg::screen_probe_kernel<64><<<grid, 64, 0, s>>>(d_x, n, w.chi, w.clo, w.meta, n_lists, w.np, d_s, d_e);
    else pg::screen_probe_kernel<128><<<grid, 64, 0, s>>>(d_x, n, w.chi, w.clo, w.meta, n_lists, w.np, d_s, d_e);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(out_s, d_s, ob, hipMemcpyDeviceToHost, s));
    PG_HIP(hipMemcpyAsync(out_e, d_e, ob, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    return PG_OK;
}
