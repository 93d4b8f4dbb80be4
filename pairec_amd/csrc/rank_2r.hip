// rank_2r.hip — the two-role DNN3 kernel: PG_PREC_BF16X3 on the bf16 matrix pipe (dnn3_x3_kernel) and PG_PREC_F16X2 /
// PG_PREC_F16 on the fp16 one (dnn3_h2_kernel), both built from one body, dnn3_two_role<Ops, H1, H2>, and an operand policy.
//
// The structure: one persistent workgroup per CU over 128-item tiles, EIGHT waves in TWO ROLES that share each SIMD:
//   * waves 0-3 ("layer-1 waves", one per SIMD): gather the tile's table rows (a tile ahead, straight to registers), convert
//     them into the X tile (one plane per activation part), and run layer 1 in chunks of 64 hidden columns — wave (mp, nb)
//     owns item blocks 2mp, 2mp + 1 and column block nb of the chunk (16 MFMAs per product: 48 in BF16X3) — then relu, convert,
//     and store the chunk into a double-buffered LDS tile.  They also finish the previous tile's scores (four partials per
//     item and head, sigmoid, store).
//   * waves 4-7 ("layer-2 waves"): wave wn keeps the fp32 accumulators of ALL 128 items x its H2 / 4 output columns for the
//     tile (128 registers at H2 = 256) and adds one chunk's 64-deep partial product per interval (32 MFMAs per product: 96
//     in BF16X3); at the end of the tile: relu → dot with every head's w3 from the accumulators → one partial per (item,
//     head, wave).
//   One barrier per chunk.  The two waves of a SIMD run different code between the same barriers, so one's LDS reads, global
//   loads and conversions sit under the other's MFMAs without any hand-made interleaving — and the matrix pipe sees
//   both waves' MFMAs per SIMD and interval (48 + 96 in BF16X3) whichever wave issues them.
//   Weights (768 KB at 512-256 in BF16X3: every matrix as hi and lo fragments) do not fit the CU: they stream from L2 once per
//   tile, global → registers, each fragment a k-step (layer 2) or a chunk (layer 1) ahead of its use.  A layer-2 fragment
//   feeds four item blocks (BF16X3's hi fragments twice: 6 / 3 MFMAs per 1-KiB load).
//   What a mode supplies (X3Ops, H2Ops<NPROD> below): the fragment type and MFMA, the number of activation planes in LDS,
//   the products of a k-step as (weight part, activation plane) pairs in issue order, and the two convert-and-store steps.
//   What only the fp16 modes have (the scale factors, the range flag, the fallback list) sits behind `Ops::kScaled` — the
//   order in which a thread walks its quads in the two store steps included: the scaled modes go quad by quad, so that one
//   load of the factors serves both passes / item blocks; BF16X3 keeps the pass-major order its schedule was measured with.
//
// ---- PG_PREC_BF16X3 ("split bf16"): the fp32 specification on the bf16 matrix pipe ----
// Why the mode exists: the reference hands model outputs on as fp32 widened to f64 (algorithm/eas/easyrec_response.go:479-483,
// eas/tf_response.go:55-59) and north_star asks for scores within 1e-5 of that path.  PG_PREC_BF16 misses it (4e-5), the fp32
// MFMA meets it at 1/16 of the bf16 rate.  Here every operand of the two matrix layers is a pair of bf16 values, x = hi + lo,
// and a term is three products — lo_w·hi_x, hi_w·lo_x, hi_w·hi_x — into the fp32 accumulator: 2^-16 relative per product,
// scores within ~1e-7 of PG_PREC_F32's, three times the MFMA work of the bf16 mode.
// LDS: X hi / lo 64 KB + two H1 chunks hi / lo 64 KB + the request's layer-1 partial, b2, the heads' w3 and partials.
// Where it stands (round 5, cycle stamps and ablation builds, since retired): the matrix pipe is 61 %
// busy at the 1.95 GHz the chip holds under this kernel.  An interval is 6.3-6.7 K cycles for 4.6 K of MFMA issue per SIMD;
// the layer-1 wave is its critical path (48 MFMAs + conversion: 2.9 K cycles with the pipe to itself, 5.4-6.8 K beside the
// layer-2 wave's 96 MFMAs).  Tried and dropped, all bit-identical, none faster than 1.18-1.20 ms: the conversion of chunk
// c under the MFMAs of chunk c + 1 (second accumulator set, layer-2 waves two intervals behind; as a block per k-step, and
// cut into pieces between the individual MFMAs), weight fragments re-requested per k-step, weight fragments two k-steps
// ahead in the layer-2 waves, priority to the layer-2 waves (-3 %).
// Round 6 (same box, `scripts/dev/x3_time.py`, ablation builds, since retired): 1.205 ms; X stored UNSPLIT (ablation 1 = the
// most a pre-split hi / lo shadow of the table rows could save): 1.23; H1 stored with NO relu / split at all (ablation 3): 1.19; X
// fragments two k-steps ahead: 1.205.  The conversions are not what the kernel waits for, and neither is the matrix pipe's schedule:
// rocm-smi beside a loop of this kernel reads 1 377-1 381 W of the 1 400 W package limit at 2.04-2.09 GHz of 2.4 (`scripts/dev/
// power_probe.sh`, bench.py's `power` object) — the kernel runs at the power limit, a busier pipe gets a lower clock.
//
// ---- PG_PREC_F16X2 / PG_PREC_F16: the fp32 specification to 1e-5 on the fp16 matrix pipe ----
// Why the modes exist: PG_PREC_BF16X3 pays three bf16 products per term for 1.2e-7 where north_star asks for 1e-5.  fp16 has the
// bf16 MFMA rate and a unit round-off of 2^-11 instead of 2^-8: activations rounded ONCE to fp16 and weights as hi + lo fp16
// (F16X2, two products per term) or rounded once as well (F16, one product) stay within ~3e-6 / ~4e-6 of the fp32 scores
// (tests/test_f16_modes_cpu.py is the numpy statement of both).  What fp16 lacks is range, so every operand is scaled by an
// exact power of two at load time (pg_model_load: build_f16_operands, rank_model.hpp):
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
// Against BF16X3: v_mfma_f32_32x32x16_f16 with ONE fp16 plane for the X tile (32 KB) and the two H1 chunk buffers (32 KB),
// NPROD MFMAs per accumulator and k-step instead of three and NPROD / 3 of the weight-fragment traffic.
#include "rank_mlp.hpp"

namespace pg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

#define TR_READY2(a0, a1) asm volatile("s_nop 3" : "+v"(a0), "+v"(a1))
#define TR_DONE2(a0, a1) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a0), "+v"(a1))
#define TR_READY1(a0) asm volatile("s_nop 3" : "+v"(a0))
#define TR_DONE1(a0) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a0))

constexpr int k2rItems = 128;
constexpr int k2rCH = 64;
constexpr int k2rXB = k2rItems * kDIN * 2;      // one plane of the X tile
constexpr int k2rHCB = k2rItems * k2rCH * 2;    // one plane of an H1 chunk buffer

__device__ __forceinline__ float relu(float v) { return __builtin_amdgcn_fmed3f(v, 0.0f, __builtin_inff()); }

// 4 consecutive columns of one row of an H1 chunk tile: 128-B rows, quads keyed by (row >> 1) & 7 (see ls_store_h_quad in
// rank_rs.hip)
__device__ __forceinline__ char* h_quad(char* tile, int row, int col) {
    return tile + row * 128 + ((((col >> 3) ^ ((row >> 1) & 7))) << 4) + (col & 7) * 2;
}

// one MFMA of a k-step: weight part (0 = hi, 1 = lo) against activation plane (0 = hi or the only one, 1 = lo)
struct Prod { int w, x; };

// PG_PREC_BF16X3: hi and lo planes of everything, three products; no scaling, no range to watch
struct X3Ops {
    typedef bf16x8 Frag;
    struct Seen {};
    static constexpr bool kScaled = false;
    static constexpr int kPlanes = 2, kWParts = 2, kNProd = 3;
    static constexpr Prod kProd[3] = {{1, 0}, {0, 1}, {0, 0}};
    static __device__ __forceinline__ void mfma(f32x16& acc, Frag b, Frag x) {
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(b), "v"(x));
    }
    static __device__ __forceinline__ void store_x(char* tile, int row, int c, float4 v, float4, Seen&) {
        store_x_quad<2>(tile, row, c, v, k2rXB);
    }
    // relu → split; the lo tile lies a plane on
    static __device__ __forceinline__ void store_h(char* tile, int row, int col, float v0, float v1, float v2, float v3, float4, Seen&) {
        uint2 ph, pl;
        split_bf16x2(relu(v0), relu(v1), ph.x, pl.x);
        split_bf16x2(relu(v2), relu(v3), ph.y, pl.y);
        char* const d = h_quad(tile, row, col);
        *reinterpret_cast<uint2*>(d) = ph;
        *reinterpret_cast<uint2*>(d + k2rHCB) = pl;
    }
};

// PG_PREC_F16X2 (NPROD 2) / PG_PREC_F16 (NPROD 1): one fp16 activation plane, scaled in front of the convert
template <int NPROD>
struct H2Ops {
    static_assert(NPROD == 1 || NPROD == 2, "one or two fp16 products per term");
    typedef f16x8 Frag;
    typedef u16x2 Seen;                         // the largest |half| bit pattern so far (0x7c00 and above: inf / NaN)
    static constexpr bool kScaled = true;
    static constexpr int kPlanes = 1, kWParts = NPROD, kNProd = NPROD;
    static constexpr Prod kProd[2] = {{NPROD - 1, 0}, {0, 0}};   // (lo_w, x), (hi_w, x) — or (hi_w, x) alone
    static __device__ __forceinline__ void mfma(f32x16& acc, Frag b, Frag x) {
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(b), "v"(x));
    }
    // two fp32 → one packed fp16 pair (RNE)
    static __device__ __forceinline__ uint32_t pack(float a, float b, Seen& seen) {
        typedef float f32x2_ __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
        const f32x2_ v = {a, b};
        const uint32_t p = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_));
        seen = __builtin_elementwise_max(seen, __builtin_bit_cast(u16x2, p & 0x7fff7fffu));
        return p;
    }
    static __device__ __forceinline__ bool out_of_range(Seen seen) { return seen.x >= 0x7c00 || seen.y >= 0x7c00; }
    // scale by the columns' factors `f` → fp16
    static __device__ __forceinline__ void store_x(char* tile, int row, int c, float4 v, float4 f, Seen& seen) {
        uint2 pk;
        pk.x = pack(v.x * f.x, v.y * f.y, seen);
        pk.y = pack(v.z * f.z, v.w * f.w, seen);
        *reinterpret_cast<uint2*>(tile + row * 256 + ((((c >> 1) ^ (row & 15))) << 4) + (c & 1) * 8) = pk;
    }
    // relu → scale by the units' factors `f` → fp16
    static __device__ __forceinline__ void store_h(char* tile, int row, int col, float v0, float v1, float v2, float v3, float4 f, Seen& seen) {
        uint2 pk;
        pk.x = pack(relu(v0) * f.x, relu(v1) * f.y, seen);
        pk.y = pack(relu(v2) * f.z, relu(v3) * f.w, seen);
        *reinterpret_cast<uint2*>(h_quad(tile, row, col)) = pk;
    }
};

template <class Ops, int H1, int H2>
constexpr size_t lds_bytes(uint32_t n_out) {
    return (size_t)Ops::kPlanes * (k2rXB + 2 * k2rHCB) +
           (size_t)(H1 + H2 + n_out * H2 + kMaxHeads + n_out * 4 * k2rItems + (Ops::kScaled ? H1 + kDIN + 4 : 0)) * 4;
}

template <class Ops, int H1, int H2>
__device__ __forceinline__ void dnn3_two_role(const MlpArgs& a) {
    typedef typename Ops::Frag Frag;
    typedef typename Ops::Seen Seen;
    constexpr int M = k2rItems, CH = k2rCH, NCH = H1 / CH, KS1 = kDIN / 16, KS2 = H1 / 16, KSC = CH / 16, NB2 = H2 / 128;
    constexpr int X_B = k2rXB, HC_B = k2rHCB, PL = Ops::kPlanes, WP = Ops::kWParts, NP = Ops::kNProd;
    static_assert(H2 == 128 || H2 == 256, "four layer-2 waves x one or two 32-column blocks");
    static_assert(NCH >= 2 && KSC == 4, "chunks");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const XT = smem;                                  // X tile: plane p lies p * X_B on
    char* const HC = smem + PL * X_B;                       // H1 chunk buffers [2][PL planes]
    float* const c1s = reinterpret_cast<float*>(smem + PL * (X_B + 2 * HC_B));   // the request's layer-1 partial (* 2^S)
    float* const hss = c1s + H1;                            // scaled only: 2^(F_i + G - S) per hidden unit
    float* const xss = hss + H1;                            // scaled only: 2^(E_k + G) per input column
    float* const b2s = Ops::kScaled ? xss + kDIN : c1s + H1;   // b2 (* 2^S)
    const uint32_t n_out = a.n_out;
    float* const w3s = b2s + H2;                            // [n_out][H2] (* 2^-S)
    float* const b3s = w3s + n_out * H2;                    // [kMaxHeads]
    float* const hps = b3s + kMaxHeads;                     // head partials [n_out][4 waves][128 items]
    uint32_t* const marks = reinterpret_cast<uint32_t*>(hps + n_out * 4 * M);   // scaled only: [2], tile parity → out of range
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_tiles = *a.n_tiles;
    const uint32_t t_begin = (uint32_t)(((uint64_t)n_tiles * blockIdx.x) / gridDim.x);
    const uint32_t t_end = (uint32_t)(((uint64_t)n_tiles * (blockIdx.x + 1)) / gridDim.x);
    if (t_begin >= t_end) return;
    for (int i = tid; i < H2; i += 512) {
        for (uint32_t o = 0; o < n_out; ++o) {
            if constexpr (Ops::kScaled) w3s[o * H2 + i] = a.w3[o * H2 + i] * a.f16_unscale;
            else w3s[o * H2 + i] = a.w3[o * H2 + i];
        }
        if constexpr (Ops::kScaled) b2s[i] = a.b2[i] * a.f16_scale;
        else b2s[i] = a.b2[i];
    }
    if constexpr (Ops::kScaled) {
        for (int i = tid; i < H1; i += 512) hss[i] = a.f16_hs[i];
        if (tid < kDIN) xss[tid] = a.f16_xs[tid];
    }
    if (tid < (int)n_out) b3s[tid] = a.b3v[tid];
    if constexpr (Ops::kScaled) {
        if (tid < 2) marks[tid] = 0;
        if (tid == 0) atomicAdd(a.f16_stats, (unsigned long long)(t_end - t_begin));
        __syncthreads();
    }

    if (wave < 4) {
        // =========================================== layer-1 waves ===========================================
        // the layer-1 wave's MFMAs first: its relu / convert / store then runs under the other wave's MFMAs (+1 %; the other
        // way round costs 3 %)
        asm volatile("s_setprio 2");
        const int mp = wave & 1, nb1 = wave >> 1;
        const char* const w1_base[2] = {reinterpret_cast<const char*>(a.w1p), reinterpret_cast<const char*>(a.w1p_lo)};
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
        // scaled only: a wave that saw an out-of-range value marks the tile of parity `par`
        auto mark = [&](Seen seen, uint32_t par) {
            if constexpr (Ops::kScaled)
                if (__builtin_amdgcn_ballot_w64(Ops::out_of_range(seen)) != 0 && (threadIdx.x & 63) == 0) marks[par] = 1;
        };
        uint32_t c1_req = 0xffffffffu;
        // X tile (scaled: per column) + the request's layer-1 partial (the X tile is idle)
        auto write_x = [&](const Tile& d, uint32_t par) {
            if (d.cnt == 0) return;
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            Seen seen{};
            if constexpr (Ops::kScaled) {                   // quad by quad: one load of the columns' factors serves both passes
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 4 * j + (t_ & 3);
                    const float4 f = *reinterpret_cast<const float4*>(xss + 4 * c);
#pragma unroll
                    for (int p = 0; p < 2; ++p) Ops::store_x(XT, p * 64 + (t_ >> 2), c, xq[p][j], f, seen);
                }
            } else {
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int j = 0; j < 8; ++j) Ops::store_x(XT, p * 64 + (t_ >> 2), 4 * j + (t_ & 3), xq[p][j], float4{}, seen);
            }
            if constexpr (Ops::kScaled) mark(seen, par);
            if (d.req != c1_req) {
                c1_req = d.req;
                for (int i = t_; i < H1; i += 256) {
                    if constexpr (Ops::kScaled) c1s[i] = a.c1[(size_t)d.req * a.c1_stride + i] * a.f16_scale;
                    else c1s[i] = a.c1[(size_t)d.req * a.c1_stride + i];
                }
            }
        };
        // a finished tile's scores: z = b3 + the four layer-2 waves' partials in wave order; thread (item, head parity).
        // Scaled: a marked tile goes onto the fallback list (its scores here are then overwritten).
        auto finalize = [&](const Tile& f, uint32_t par) {
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            if constexpr (Ops::kScaled) {
                if (t_ == 0 && marks[par]) {
                    marks[par] = 0;
                    const uint32_t slot = atomicAdd(a.fb_n_tiles, 1u);
                    a.fb_tile_req[slot] = f.req;
                    a.fb_tile_item0[slot] = f.item0;
                    a.fb_tile_cnt[slot] = f.cnt;
                    atomicAdd(a.f16_stats + 1, 1ull);
                }
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
        Frag w1[WP][KS1];
        auto load_w1 = [&](int c) {                         // fragments of n-block c * 2 + nb1, every k-step, every part
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((c * 2 + nb1) * KS1 * 1024);
            uint32_t l_ = threadIdx.x;
            asm volatile("" : "+v"(l_));
            const uint32_t lane_off = (l_ & 63) * 16;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
                for (int w = 0; w < WP; ++w) w1[w][ks] = *reinterpret_cast<const Frag*>(w1_base[w] + off + ks * 1024 + lane_off);
        };

        Tile cur = load_desc(t_begin), fin{0, 0, 0};
        uint32_t par = 0;                                   // scaled only: parity of `cur` within this workgroup's run of tiles
        gather(cur);
        load_w1(0);
        write_x(cur, par);
        __syncthreads();                                    // prologue barrier
        for (uint32_t tile = t_begin; tile < t_end; ++tile) {
            const Tile nxt = load_desc(tile + 1);
            gather(nxt);                                    // lands during the tile, stored behind its last chunk
            Seen seen{};
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
                TR_READY2(acc[0], acc[1]);
                const char* const xr0 = XT + ((2 * mp) * 32 + i32) * 256;
                const char* const xr1 = xr0 + 32 * 256;
                Frag xf[2][PL][2];                          // [slot][plane][item block]
                auto xfrag = [&](int ks, int s) {
                    const int q = ((ks * 2 + h) ^ (i32 & 15)) << 4;
#pragma unroll
                    for (int p = 0; p < PL; ++p) {
                        xf[s][p][0] = *reinterpret_cast<const Frag*>(xr0 + p * X_B + q);
                        xf[s][p][1] = *reinterpret_cast<const Frag*>(xr1 + p * X_B + q);
                    }
                };
                xfrag(0, 0);
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    if (ks + 1 < KS1) xfrag(ks + 1, (ks + 1) & 1);
#pragma unroll
                    for (int i = 0; i < NP; ++i)
#pragma unroll
                        for (int mb = 0; mb < 2; ++mb) Ops::mfma(acc[mb], w1[Ops::kProd[i].w][ks], xf[ks & 1][Ops::kProd[i].x][mb]);
                }
                load_w1(c + 1 < NCH ? c + 1 : 0);           // next chunk's (next tile's first) fragments
                TR_DONE2(acc[0], acc[1]);
                // relu → (scaled: unit factor) → convert → the chunk tile
                char* const hb = HC + (c & 1) * (PL * HC_B);
                if constexpr (Ops::kScaled) {               // quad by quad, as in write_x
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int col = nb1 * 32 + 8 * g + 4 * h;
                        const float4 f = *reinterpret_cast<const float4*>(hss + c * CH + col);
#pragma unroll
                        for (int mb = 0; mb < 2; ++mb)
                            Ops::store_h(hb, (2 * mp + mb) * 32 + i32, col, acc[mb][4 * g + 0], acc[mb][4 * g + 1],
                                         acc[mb][4 * g + 2], acc[mb][4 * g + 3], f, seen);
                    }
                } else {
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            Ops::store_h(hb, (2 * mp + mb) * 32 + i32, nb1 * 32 + 8 * g + 4 * h, acc[mb][4 * g + 0],
                                         acc[mb][4 * g + 1], acc[mb][4 * g + 2], acc[mb][4 * g + 3], float4{}, seen);
                }
                if constexpr (Ops::kScaled)
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
        const char* const w2_base[2] = {reinterpret_cast<const char*>(a.w2p) + (size_t)(wn * NB2) * KS2 * 1024,
                                        reinterpret_cast<const char*>(a.w2p_lo) + (size_t)(wn * NB2) * KS2 * 1024};
        f32x16 acc2[4][NB2];
        Frag w2[2][WP][NB2];                                // [slot][part][column block]
        auto load_w2 = [&](int kk, int s) {
            uint32_t l_ = threadIdx.x;
            asm volatile("" : "+v"(l_));
            const uint32_t lane_off = (l_ & 63) * 16;
#pragma unroll
            for (int nb = 0; nb < NB2; ++nb)
#pragma unroll
                for (int w = 0; w < WP; ++w)
                    w2[s][w][nb] = *reinterpret_cast<const Frag*>(w2_base[w] + (uint32_t)((nb * KS2 + kk) * 1024) + lane_off);
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
                if constexpr (NB2 == 2) TR_READY2(acc2[mb][0], acc2[mb][1]);
                else TR_READY1(acc2[mb][0]);
            }
        };
        // relu → dot with every head's w3 (scaled: held * 2^-S) over this wave's columns: one partial per (head, item); a
        // lane owns 16 * NB2 of its item's columns, lanes i and i + 32 the two column halves of a block
        auto head = [&]() {
            uint32_t t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            const int i32 = t_ & 31, h = (t_ >> 5) & 1;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                if constexpr (NB2 == 2) TR_DONE2(acc2[mb][0], acc2[mb][1]);
                else TR_DONE1(acc2[mb][0]);
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
                const char* const hr = HC + (c & 1) * (PL * HC_B) + i32 * 128;
                const int sw = (i32 >> 1) & 7;
                // A fragments (every plane) of step f = (k-step f / 4, item block f % 4): three ahead in four rotating slots
                Frag af[4][PL];
                auto afrag = [&](int f) {
                    const char* const p = hr + (f & 3) * (32 * 128) + ((((f >> 2) * 2 + h) ^ sw) << 4);
#pragma unroll
                    for (int pl = 0; pl < PL; ++pl) af[f & 3][pl] = *reinterpret_cast<const Frag*>(p + pl * HC_B);
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
#pragma unroll
                    for (int i = 0; i < NP; ++i)
#pragma unroll
                        for (int nb = 0; nb < NB2; ++nb)
                            Ops::mfma(acc2[mb][nb], w2[ks & 1][Ops::kProd[i].w][nb], af[f & 3][Ops::kProd[i].x]);
                }
                __syncthreads();
            }
        }
        head();
        __syncthreads();
    }
}

template <int H1, int H2>
__global__ __launch_bounds__(512, 1) void dnn3_x3_kernel(MlpArgs a) {
    dnn3_two_role<X3Ops, H1, H2>(a);
}

template <int H1, int H2, int NPROD>
__global__ __launch_bounds__(512, 1) void dnn3_h2_kernel(MlpArgs a) {
    dnn3_two_role<H2Ops<NPROD>, H1, H2>(a);
}

template <class Ops, int H1, int H2>
static int launch_2r(pg_ctx* ctx, void (*kernel)(MlpArgs), const MlpArgs& a) {
    const size_t lds = lds_bytes<Ops, H1, H2>(a.n_out);
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)kernel, lds))) return rc;
    kernel<<<ctx->num_cus, 512, lds, ctx->stream>>>(a);
    return PG_OK;
}

#define PG_2R_SHAPES(X) X(512, 256) X(256, 256) X(256, 128) X(128, 128)

bool dnn3_x3_shape(uint32_t h1, uint32_t h2) {
#define X(A, B) if (h1 == A && h2 == B) return true;
    PG_2R_SHAPES(X)
#undef X
    return false;
}

int launch_dnn3_x3(pg_ctx* ctx, uint32_t h1, uint32_t h2, const MlpArgs& a) {
#define X(A, B) if (h1 == A && h2 == B) return launch_2r<X3Ops, A, B>(ctx, dnn3_x3_kernel<A, B>, a);
    PG_2R_SHAPES(X)
#undef X
    set_error("rank: no split-bf16 kernel for hidden widths %u-%u", h1, h2);
    return PG_ERR_UNSUPPORTED;
}

int launch_dnn3_h2(pg_ctx* ctx, uint32_t h1, uint32_t h2, int nprod, const MlpArgs& a) {
    if (nprod != 1 && nprod != 2) {
        set_error("rank: an fp16 mode has one or two products per term, not %d", nprod);
        return PG_ERR_INVALID;
    }
#define X(A, B)                                                                                              \
    if (h1 == A && h2 == B)                                                                                  \
        return nprod == 2 ? launch_2r<H2Ops<2>, A, B>(ctx, dnn3_h2_kernel<A, B, 2>, a)                      \
                          : launch_2r<H2Ops<1>, A, B>(ctx, dnn3_h2_kernel<A, B, 1>, a);
    PG_2R_SHAPES(X)
#undef X
    set_error("rank: no fp16 kernel for hidden widths %u-%u", h1, h2);
    return PG_ERR_UNSUPPORTED;
}

}  // namespace pg
