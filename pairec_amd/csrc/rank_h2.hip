// rank_h2.hip — DNN3 in PG_PREC_F16X2 / PG_PREC_F16: the fp32 specification to 1e-5 on the fp16 matrix pipe.
//
// Why the modes exist: PG_PREC_BF16X3 pays three bf16 products per term for 1.2e-7 where north_star asks for 1e-5.  fp16 has the
// bf16 MFMA rate and a unit round-off of 2^-11 instead of 2^-8: activations rounded ONCE to fp16 and weights as hi + lo fp16
// (F16X2, two products per term) or rounded once as well (F16, one product) stay within ~3e-6 / ~4e-6 of the fp32 scores
// (tests/test_f16_modes_cpu.py is the numpy statement of both).  What fp16 lacks is range, so every operand is scaled by an
// exact power of two at load time (pg_model_load, rank_mlp.hip):
//   E_k = floor(log2 max_j |W1[k][j]|)   per input column k of layer 1's item half   (0 for an all-zero row)
//   F_i = floor(log2 max_j |W2[i][j]|)   per hidden unit i                           (0 for an all-zero row)
//   "row-normalised units": wn = W * 2^-E (row maximum in [1, 2)), xn_k = x_k * 2^E_k — the products are unchanged.
//   the kernel feeds      x'_k = x_k * 2^(E_k + G)                  (xs[k], one multiply in front of the fp16 convert)
//   against               W1'[k][j] = W1[k][j] * 2^(-E_k - G + S)   → layer-1 accumulators hold 2^S * z1 (c1 enters as c1 * 2^S)
//   then                  h'_i = relu(acc1_i) * 2^(F_i + G - S)     (hs[i], one multiply in front of the fp16 convert)
//   against               W2'[i][j] = W2[i][j] * 2^(-F_i - G + S)   → layer-2 accumulators hold 2^S * z2 (b2 enters as b2 * 2^S);
//   S is undone exactly where those are read: the heads' w3 are held as w3 * 2^-S.
//   G = kH2G = 11, S = kH2S = 23.  S - G = 12 puts every weight row's maximum in [2^12, 2^13): its lo part is at most 2, and
//   whatever of a lo part falls under fp16's smallest normal 2^-14 is at most 2^-26 of the row maximum.  (The unit factor
//   2^(F_i + G) cannot be folded into W1's column i under one S — F_i - E_k would have to stay inside five octaves for the
//   lo parts to stay normal — so it is the multiply that also undoes S.)
//   Nothing here assumes that the matrix pipe keeps fp16 subnormal operands.  A scaled activation under 2^-14 is, at
//   worst, flushed to zero: |xn| < 2^(-14 - G) = 2^-25, against a normalised weight below 2, is a term error below 2^-24 —
//   a pre-activation errs by at most fan_in * 2^-24 absolutely whatever the table holds (128 * 2^-24 = 7.6e-6 in the one
//   case where every column underflows at once; kept subnormals err 2^-36 instead).  The price is the overflow threshold: a
//   scaled activation beyond 65504 — a single normalised activation of 2^(16 - G) = 32 and more — is out of range.
// Range flag and fallback: a layer-1 wave that sees a scaled x or h1 whose fp16 is inf or NaN marks its tile; the tile's
// descriptor (req, item0, cnt) is appended to a compact list (one atomic on the call's counter, one on the model's total), and
// rank_dnn3_dev_locked enqueues dnn3_x3_kernel over that list directly behind this kernel — n_tiles read from the device
// counter, no host synchronisation — which overwrites the marked tiles with PG_PREC_BF16X3's scores.
//
// dnn3_h2_kernel is dnn3_x3_kernel's structure (rank_x3.hip: one persistent workgroup per CU, 128-item tiles, four layer-1
// and four layer-2 waves sharing the SIMDs, one barrier per 64-column chunk) on v_mfma_f32_32x32x16_f16 with ONE fp16 plane
// for the X tile (32 KB) and the two H1 chunk buffers (32 KB), NPROD MFMAs per accumulator and k-step instead of three and
// NPROD / 3 of the weight-fragment traffic.
#include "rank_mlp.hpp"

namespace pg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

#define H2_MFMA(acc, b, x) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(b), "v"(x))
#define H2_READY2(a0, a1) asm volatile("s_nop 3" : "+v"(a0), "+v"(a1))
#define H2_DONE2(a0, a1) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a0), "+v"(a1))
#define H2_READY1(a0) asm volatile("s_nop 3" : "+v"(a0))
#define H2_DONE1(a0) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a0))

constexpr int kH2Items = 128;
constexpr int kH2CH = 64;

template <int H1, int H2>
constexpr size_t h2_lds_bytes(uint32_t n_out) {
    return (size_t)kH2Items * kDIN * 2 + (size_t)2 * kH2Items * kH2CH * 2 +
           (size_t)(2 * H1 + kDIN + H2 + n_out * H2 + kMaxHeads + n_out * 4 * kH2Items + 4) * 4;
}

// two fp32 → one packed fp16 pair (RNE); `seen` keeps the largest |half| bit pattern (0x7c00 and above: inf / NaN)
__device__ __forceinline__ uint32_t h2_pack(float a, float b, u16x2& seen) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
    const f32x2_ v = {a, b};
    const uint32_t p = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_));
    seen = __builtin_elementwise_max(seen, __builtin_bit_cast(u16x2, p & 0x7fff7fffu));
    return p;
}
__device__ __forceinline__ bool h2_out_of_range(u16x2 seen) { return seen.x >= 0x7c00 || seen.y >= 0x7c00; }

__device__ __forceinline__ float h2_relu(float v) { return __builtin_amdgcn_fmed3f(v, 0.0f, __builtin_inff()); }

template <int H1, int H2, int NPROD>
__global__ __launch_bounds__(512, 1) void dnn3_h2_kernel(MlpArgs a) {
    constexpr int M = kH2Items, CH = kH2CH, NCH = H1 / CH, KS1 = kDIN / 16, KS2 = H1 / 16, KSC = CH / 16, NB2 = H2 / 128;
    constexpr int X_B = M * kDIN * 2, HC_B = M * CH * 2;
    static_assert(H2 == 128 || H2 == 256, "four layer-2 waves x one or two 32-column blocks");
    static_assert(NCH >= 2 && KSC == 4, "chunks");
    static_assert(NPROD == 1 || NPROD == 2, "one or two fp16 products per term");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const XT = smem;                                  // X tile, one fp16 plane
    char* const HC = smem + X_B;                            // H1 chunk buffers [2]
    float* const c1s = reinterpret_cast<float*>(smem + X_B + 2 * HC_B);   // the request's layer-1 partial * 2^S
    float* const hss = c1s + H1;                            // 2^(F_i + G - S) per hidden unit
    float* const xss = hss + H1;                            // 2^(E_k + G) per input column
    float* const b2s = xss + kDIN;                          // b2 * 2^S
    const uint32_t n_out = a.n_out;
    float* const w3s = b2s + H2;                            // [n_out][H2], * 2^-S
    float* const b3s = w3s + n_out * H2;                    // [kMaxHeads]
    float* const hps = b3s + kMaxHeads;                     // head partials [n_out][4 waves][128 items]
    uint32_t* const marks = reinterpret_cast<uint32_t*>(hps + n_out * 4 * M);   // [2]: tile parity → out of range
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_tiles = *a.n_tiles;
    const uint32_t t_begin = (uint32_t)(((uint64_t)n_tiles * blockIdx.x) / gridDim.x);
    const uint32_t t_end = (uint32_t)(((uint64_t)n_tiles * (blockIdx.x + 1)) / gridDim.x);
    if (t_begin >= t_end) return;
    for (int i = tid; i < H2; i += 512) {
        for (uint32_t o = 0; o < n_out; ++o) w3s[o * H2 + i] = a.w3[o * H2 + i] * a.f16_unscale;
        b2s[i] = a.b2[i] * a.f16_scale;
    }
    for (int i = tid; i < H1; i += 512) hss[i] = a.f16_hs[i];
    if (tid < kDIN) xss[tid] = a.f16_xs[tid];
    if (tid < (int)n_out) b3s[tid] = a.b3v[tid];
    if (tid < 2) marks[tid] = 0;
    if (tid == 0) atomicAdd(a.f16_stats, (unsigned long long)(t_end - t_begin));
    __syncthreads();

    if (wave < 4) {
        // =========================================== layer-1 waves ===========================================
        asm volatile("s_setprio 2");
        const int mp = wave & 1, nb1 = wave >> 1;
        const char* const w1h_base = reinterpret_cast<const char*>(a.w1p);
        const char* const w1l_base = reinterpret_cast<const char*>(a.w1p_lo);
        struct Tile { uint32_t req, item0, cnt; };
        auto load_desc = [&](uint32_t t) {
            Tile d{0, 0, 0};
            if (t < t_end) {
                d.req = (uint32_t)__builtin_amdgcn_readfirstlane(a.tile_req[t]);
                d.item0 = (uint32_t)__builtin_amdgcn_readfirstlane(a.tile_item0[t]);
                d.cnt = (uint32_t)__builtin_amdgcn_readfirstlane(a.tile_cnt[t]);
            }
            return d;
        };
        // gather: 4 adjacent lanes per item (64 contiguous bytes per instruction), two passes of 64 items
        float4 xq[2][8];
        auto gather = [&](const Tile& d) {
            if (d.cnt == 0) return;
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const uint32_t item = p * 64 + (t_ >> 2);
                uint32_t row = a.cand_rows[d.item0 + (item < d.cnt ? item : d.cnt - 1)];
                row = row < a.tab_rows ? row : a.tab_rows - 1;
                const float4* src = reinterpret_cast<const float4*>(a.tab + (size_t)row * kDIN) + (t_ & 3);
#pragma unroll
                for (int j = 0; j < 8; ++j) xq[p][j] = src[4 * j];
            }
        };
        // a wave that saw an out-of-range value marks the tile of parity `par`
        auto mark = [&](u16x2 seen, uint32_t par) {
            if (__builtin_amdgcn_ballot_w64(h2_out_of_range(seen)) != 0 && (threadIdx.x & 63) == 0) marks[par] = 1;
        };
        uint32_t c1_req = 0xffffffffu;
        // X tile (scaled per column, fp16) + the request's layer-1 partial (the X tile is idle)
        auto write_x = [&](const Tile& d, uint32_t par) {
            if (d.cnt == 0) return;
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            u16x2 seen = {0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 4 * j + (t_ & 3);
                const float4 f = *reinterpret_cast<const float4*>(xss + 4 * c);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int row = p * 64 + (t_ >> 2);
                    const float4 v = xq[p][j];
                    uint2 pk;
                    pk.x = h2_pack(v.x * f.x, v.y * f.y, seen);
                    pk.y = h2_pack(v.z * f.z, v.w * f.w, seen);
                    *reinterpret_cast<uint2*>(XT + row * 256 + ((((c >> 1) ^ (row & 15))) << 4) + (c & 1) * 8) = pk;
                }
            }
            mark(seen, par);
            if (d.req != c1_req) {
                c1_req = d.req;
                for (int i = t_; i < H1; i += 256) c1s[i] = a.c1[(size_t)d.req * a.c1_stride + i] * a.f16_scale;
            }
        };
        // a finished tile's scores: z = b3 + the four layer-2 waves' partials in wave order; thread (item, head parity).
        // A marked tile goes onto the fallback list (its scores here are then overwritten).
        auto finalize = [&](const Tile& f, uint32_t par) {
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            if (t_ == 0 && marks[par]) {
                marks[par] = 0;
                const uint32_t slot = atomicAdd(a.fb_n_tiles, 1u);
                a.fb_tile_req[slot] = f.req;
                a.fb_tile_item0[slot] = f.item0;
                a.fb_tile_cnt[slot] = f.cnt;
                atomicAdd(a.f16_stats + 1, 1ull);
            }
            const uint32_t item = t_ & (M - 1);
            if (item < f.cnt)
                for (uint32_t o = t_ >> 7; o < n_out; o += 2) {
                    float z = b3s[o];
#pragma unroll
                    for (int s = 0; s < 4; ++s) z += hps[(o * 4 + s) * M + item];
                    a.out[(size_t)o * a.out_stride + f.item0 + item] = 1.0f / (1.0f + expf(-z));
                }
        };
        f16x8 w1h[KS1], w1l[NPROD == 2 ? KS1 : 1];
        auto load_w1 = [&](int c) {                         // fragments of n-block c * 2 + nb1, every k-step, hi (and lo)
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((c * 2 + nb1) * KS1 * 1024);
            uint32_t l_ = threadIdx.x;
            asm volatile("" : "+v"(l_));
            const uint32_t lane_off = (l_ & 63) * 16;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                w1h[ks] = *reinterpret_cast<const f16x8*>(w1h_base + off + ks * 1024 + lane_off);
                if constexpr (NPROD == 2) w1l[ks] = *reinterpret_cast<const f16x8*>(w1l_base + off + ks * 1024 + lane_off);
            }
        };

        Tile cur = load_desc(t_begin), fin{0, 0, 0};
        uint32_t par = 0;                                   // parity of `cur` within this workgroup's run of tiles
        gather(cur);
        load_w1(0);
        write_x(cur, par);
        __syncthreads();                                    // prologue barrier
        for (uint32_t tile = t_begin; tile < t_end; ++tile) {
            const Tile nxt = load_desc(tile + 1);
            gather(nxt);                                    // lands during the tile, stored behind its last chunk
            u16x2 seen = {0, 0};
#pragma unroll 1
            for (int c = 0; c < NCH; ++c) {
                if (c == 1 && fin.cnt) finalize(fin, par ^ 1);   // (its partials were written during interval 0)
                uint32_t t_ = threadIdx.x;
                asm volatile("" : "+v"(t_));
                const int i32 = t_ & 31, h = (t_ >> 5) & 1;
                f32x16 acc[2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cv = *reinterpret_cast<const float4*>(c1s + c * CH + nb1 * 32 + 8 * g + 4 * h);
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        acc[mb][4 * g + 0] = cv.x;
                        acc[mb][4 * g + 1] = cv.y;
                        acc[mb][4 * g + 2] = cv.z;
                        acc[mb][4 * g + 3] = cv.w;
                    }
                }
                H2_READY2(acc[0], acc[1]);
                const char* const xr0 = XT + ((2 * mp) * 32 + i32) * 256;
                const char* const xr1 = xr0 + 32 * 256;
                f16x8 xf[2][2];
                auto xfrag = [&](int ks, int s) {
                    const int q = ((ks * 2 + h) ^ (i32 & 15)) << 4;
                    xf[s][0] = *reinterpret_cast<const f16x8*>(xr0 + q);
                    xf[s][1] = *reinterpret_cast<const f16x8*>(xr1 + q);
                };
                xfrag(0, 0);
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    if (ks + 1 < KS1) xfrag(ks + 1, (ks + 1) & 1);
                    if constexpr (NPROD == 2) {
                        H2_MFMA(acc[0], w1l[ks], xf[ks & 1][0]);
                        H2_MFMA(acc[1], w1l[ks], xf[ks & 1][1]);
                    }
                    H2_MFMA(acc[0], w1h[ks], xf[ks & 1][0]);
                    H2_MFMA(acc[1], w1h[ks], xf[ks & 1][1]);
                }
                load_w1(c + 1 < NCH ? c + 1 : 0);           // next chunk's (next tile's first) fragments
                H2_DONE2(acc[0], acc[1]);
                // relu → unit factor → fp16 → 4 consecutive columns of one row of the chunk tile (128-B rows, quads keyed
                // by (row >> 1) & 7, as x3_store_h_quad)
                char* const hb = HC + (c & 1) * HC_B;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = nb1 * 32 + 8 * g + 4 * h;
                    const float4 f = *reinterpret_cast<const float4*>(hss + c * CH + col);
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        const int row = (2 * mp + mb) * 32 + i32;
                        uint2 pk;
                        pk.x = h2_pack(h2_relu(acc[mb][4 * g + 0]) * f.x, h2_relu(acc[mb][4 * g + 1]) * f.y, seen);
                        pk.y = h2_pack(h2_relu(acc[mb][4 * g + 2]) * f.z, h2_relu(acc[mb][4 * g + 3]) * f.w, seen);
                        *reinterpret_cast<uint2*>(hb + row * 128 + ((((col >> 3) ^ ((row >> 1) & 7))) << 4) + (col & 7) * 2) = pk;
                    }
                }
                if (c == NCH - 1) mark(seen, par);
                __syncthreads();
            }
            write_x(nxt, par ^ 1);                          // every layer-1 wave is past its last read of this tile's X
            __syncthreads();
            fin = cur;
            cur = nxt;
            par ^= 1;
        }
        __syncthreads();                                    // the layer-2 waves' head of the last tile
        finalize(fin, par ^ 1);
    } else {
        // =========================================== layer-2 waves ===========================================
        const int wn = wave - 4;
        const char* const w2h_base = reinterpret_cast<const char*>(a.w2p) + (size_t)(wn * NB2) * KS2 * 1024;
        const char* const w2l_base = reinterpret_cast<const char*>(a.w2p_lo) + (size_t)(wn * NB2) * KS2 * 1024;
        f32x16 acc2[4][NB2];
        f16x8 bh[2][NB2], bl[2][NPROD == 2 ? NB2 : 1];
        auto load_w2 = [&](int kk, int s) {
            uint32_t l_ = threadIdx.x;
            asm volatile("" : "+v"(l_));
            const uint32_t lane_off = (l_ & 63) * 16;
#pragma unroll
            for (int nb = 0; nb < NB2; ++nb) {
                bh[s][nb] = *reinterpret_cast<const f16x8*>(w2h_base + (uint32_t)((nb * KS2 + kk) * 1024) + lane_off);
                if constexpr (NPROD == 2)
                    bl[s][nb] = *reinterpret_cast<const f16x8*>(w2l_base + (uint32_t)((nb * KS2 + kk) * 1024) + lane_off);
            }
        };
        auto init_acc = [&]() {
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            const int h = (t_ >> 5) & 1;
#pragma unroll
            for (int nb = 0; nb < NB2; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bv = *reinterpret_cast<const float4*>(b2s + (wn * NB2 + nb) * 32 + 8 * g + 4 * h);
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) {
                        acc2[mb][nb][4 * g + 0] = bv.x;
                        acc2[mb][nb][4 * g + 1] = bv.y;
                        acc2[mb][nb][4 * g + 2] = bv.z;
                        acc2[mb][nb][4 * g + 3] = bv.w;
                    }
                }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                if constexpr (NB2 == 2) H2_READY2(acc2[mb][0], acc2[mb][1]);
                else H2_READY1(acc2[mb][0]);
            }
        };
        // relu → dot with every head's w3 (held * 2^-S) over this wave's columns: one partial per (head, item); a lane owns
        // 16 * NB2 of its item's columns, lanes i and i + 32 the two column halves of a block
        auto head = [&]() {
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            const int i32 = t_ & 31, h = (t_ >> 5) & 1;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                if constexpr (NB2 == 2) H2_DONE2(acc2[mb][0], acc2[mb][1]);
                else H2_DONE1(acc2[mb][0]);
            }
            for (uint32_t o = 0; o < n_out; ++o) {
                float4 wv[NB2][4];
#pragma unroll
                for (int nb = 0; nb < NB2; ++nb)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        wv[nb][g] = *reinterpret_cast<const float4*>(w3s + o * H2 + (wn * NB2 + nb) * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    float p = 0.0f;
#pragma unroll
                    for (int nb = 0; nb < NB2; ++nb)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            p = __fmaf_rn(fmaxf(acc2[mb][nb][4 * g + 0], 0.0f), wv[nb][g].x, p);
                            p = __fmaf_rn(fmaxf(acc2[mb][nb][4 * g + 1], 0.0f), wv[nb][g].y, p);
                            p = __fmaf_rn(fmaxf(acc2[mb][nb][4 * g + 2], 0.0f), wv[nb][g].z, p);
                            p = __fmaf_rn(fmaxf(acc2[mb][nb][4 * g + 3], 0.0f), wv[nb][g].w, p);
                        }
                    p += __shfl_xor(p, 32);
                    if (h == 0) hps[(o * 4 + wn) * M + mb * 32 + i32] = p;
                }
            }
        };

        load_w2(0, 0);
        __syncthreads();                                    // prologue barrier
        for (uint32_t tile = t_begin; tile < t_end; ++tile) {
            if (tile != t_begin) head();                    // the previous tile's, under this tile's first layer-1 chunk
            init_acc();
            __syncthreads();
#pragma unroll 1
            for (int c = 0; c < NCH; ++c) {
                uint32_t t_ = threadIdx.x;
                asm volatile("" : "+v"(t_));
                const int i32 = t_ & 31, h = (t_ >> 5) & 1;
                const char* const hr = HC + (c & 1) * HC_B + i32 * 128;
                const int sw = (i32 >> 1) & 7;
                // A fragments of step f = (k-step f / 4, item block f % 4): three ahead in four rotating slots
                f16x8 af[4];
                auto afrag = [&](int f) {
                    af[f & 3] = *reinterpret_cast<const f16x8*>(hr + (f & 3) * (32 * 128) + ((((f >> 2) * 2 + h) ^ sw) << 4));
                };
                afrag(0);
                afrag(1);
                afrag(2);
#pragma unroll
                for (int f = 0; f < 4 * KSC; ++f) {
                    const int ks = f >> 2, mb = f & 3;
                    if (mb == 0) {                          // the next k-step's weight fragments (of the next chunk / tile behind the last)
                        const int kn = c * KSC + ks + 1;
                        load_w2(kn < KS2 ? kn : 0, (ks + 1) & 1);
                    }
                    if (f + 3 < 4 * KSC) afrag(f + 3);
                    if constexpr (NPROD == 2) {
#pragma unroll
                        for (int nb = 0; nb < NB2; ++nb) H2_MFMA(acc2[mb][nb], bl[ks & 1][nb], af[f & 3]);
                    }
#pragma unroll
                    for (int nb = 0; nb < NB2; ++nb) H2_MFMA(acc2[mb][nb], bh[ks & 1][nb], af[f & 3]);
                }
                __syncthreads();
            }
        }
        head();
        __syncthreads();
    }
}

template <int H1, int H2>
static int launch_h2(pg_ctx* ctx, int nprod, const MlpArgs& a) {
    const size_t lds = h2_lds_bytes<H1, H2>(a.n_out);
    int rc;
    if (nprod == 2) {
        if ((rc = ensure_dyn_lds(ctx, (const void*)dnn3_h2_kernel<H1, H2, 2>, lds))) return rc;
        dnn3_h2_kernel<H1, H2, 2><<<ctx->num_cus, 512, lds, ctx->stream>>>(a);
    } else {
        if ((rc = ensure_dyn_lds(ctx, (const void*)dnn3_h2_kernel<H1, H2, 1>, lds))) return rc;
        dnn3_h2_kernel<H1, H2, 1><<<ctx->num_cus, 512, lds, ctx->stream>>>(a);
    }
    return PG_OK;
}

int launch_dnn3_h2(pg_ctx* ctx, uint32_t h1, uint32_t h2, int nprod, const MlpArgs& a) {
    if (nprod != 1 && nprod != 2) {
        set_error("rank: an fp16 mode has one or two products per term, not %d", nprod);
        return PG_ERR_INVALID;
    }
    if (h1 == 512 && h2 == 256) return launch_h2<512, 256>(ctx, nprod, a);
    if (h1 == 256 && h2 == 256) return launch_h2<256, 256>(ctx, nprod, a);
    if (h1 == 256 && h2 == 128) return launch_h2<256, 128>(ctx, nprod, a);
    if (h1 == 128 && h2 == 128) return launch_h2<128, 128>(ctx, nprod, a);
    set_error("rank: no fp16 kernel for hidden widths %u-%u", h1, h2);
    return PG_ERR_UNSUPPORTED;
}

}  // namespace pg
