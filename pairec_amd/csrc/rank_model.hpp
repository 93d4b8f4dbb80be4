// rank_model.hpp — a rank model on the host: what a blob says (header forms, shape lists, array offsets, refusals), the
// operand rounding both sides of the boundary share, the weights packed in MFMA-fragment order, and the ordered list of what
// pg_model_load sends to the device.  HIP-free: nothing here needs a device or a context, and a refusal comes back as a status
// and its text for the caller to report (tests/rank_model_check.cpp builds this header alone with the host compiler).
// rank_entry.hip loads models through it; the rank kernels (rank_mlp.hpp) take their constants and rounding from it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pairec_gpu.h"

#ifdef __HIPCC__
#define PG_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define PG_HOST_DEVICE inline
#endif

// rank model weights resident in HBM (rank_entry.hip loads them)
struct pg_model {
    pg_model_kind kind;
    int prec;
    uint32_t d_user = 0, d_item = 0, h1 = 0, h2 = 0;           // DNN3
    uint32_t nuf = 0, nif = 0, k = 0, th = 0, to = 0, vocab = 0;  // two-tower
    float b3 = 0.f, fm_b = 0.f;
    uint32_t n_out = 1;     // DNN3: heads on the shared trunk (PG_MODEL_DNN3_MULTI; kind is stored as PG_MODEL_DNN3)
    float* b3v = nullptr;   // device [n_out] head biases (b3 = b3v[0])
    // device buffers
    float* w1u = nullptr;   // [d_user][h1] (DNN3) / uw1 (two-tower), operand-rounded fp32
    float* b1 = nullptr;    // b1 / ub1
    float* uw2 = nullptr;   // two-tower user layer 2
    float* ub2 = nullptr;
    void* w1p = nullptr;    // packed item-side layer 1
    void* w2p = nullptr;    // packed layer 2
    void* w1p_lo = nullptr; // PG_PREC_BF16X3: the lo fragments (inside the w1p / w2p allocations)
    void* w2p_lo = nullptr;
    // PG_PREC_F16X2 / PG_PREC_F16: prec is 2 (every BF16X3 buffer above is kept: the fallback) and f16_nprod 2 / 1
    int f16_nprod = 0;
    void* h_w1p = nullptr;  // scaled fp16 fragments (rank_2r.hip); the lo planes inside the same allocations
    void* h_w2p = nullptr;
    void* h_w1p_lo = nullptr;
    void* h_w2p_lo = nullptr;
    float* h_xs = nullptr;  // [kDIN] input-column factors
    float* h_hs = nullptr;  // [h1] hidden-unit factors
    unsigned long long* h_stats = nullptr;   // device [2]: tiles taken by the fp16 kernel, tiles re-served in BF16X3
    mutable uint64_t f16_calls = 0, f16_calls_whole = 0;   // under the context's lock
    pg_ctx* ctx = nullptr;
    float* c1_shared = nullptr;   // two-tower: ib1
    // PG_MODEL_DIN: the activation unit folded for rank_din.hip (fold_din_attention), fp32 [d_item][att_h] each; the trunk's
    // members above are a DNN3's whose item half is the 128 rows [e | pooled] of w1
    uint32_t att_h = 0;
    float* att_wq = nullptr;
    float* att_wk = nullptr;
    float* att_wp = nullptr;
    float* att_ba = nullptr;    // [att_h]
    float* att_wa2 = nullptr;   // [att_h]
    float att_ba2 = 0.f;
    // PG_MODEL_MMOE (rank_mmoe.hip; pack_mmoe below): n_out = n_task; the tasks padded to mm_tp = 2 or 4
    uint32_t n_expert = 0, h_e = 0, h_t = 0, mm_tp = 0;
    float* mm_wu = nullptr;     // [d_user][32 + E h_e]: the user rows of Wg and We, columns in accumulator-row order
    float* mm_bu = nullptr;     // [32 + E h_e]: bg and be in that order
    void* mm_rec = nullptr;     // the gate record, then one record per step of 16 hidden units, in MFMA fragment order
    float* mm_bt = nullptr;     // [mm_tp][h_t]
    float* mm_wo = nullptr;     // [mm_tp][h_t]
    float* mm_bo = nullptr;     // [mm_tp]
    // PG_MODEL_PLE (rank_ple.hip; pack_ple below): n_out = n_task, e_task / e_shared experts per task / shared group, h_e, h_t as
    // above; mm_wu / mm_bu ([32 + 32 pl_nrec1]), mm_rec and mm_bt / mm_wo / mm_bo ([3][h_t], [3]) hold what they hold for an MMoE
    uint32_t e_task = 0, e_shared = 0, n_level = 0, pl_nrec1 = 0;
    float* pl_be2 = nullptr;    // [pl_nrec1][32]: the second level's expert biases in accumulator-row order, record by record
    float* pl_bg2 = nullptr;    // [3][4]: the second level's task-gate biases in gate-slot order
    // PG_MODEL_DCN (rank_dcn.hip; pack_dcn below): n_cross layers over x_0 padded to dc_dp columns, item columns first; the
    // head's b1, b2, w3 ([n_out][h2]) and b3v are the members a DNN3 uses
    uint32_t n_cross = 0, dc_dp = 0;
    float* dc_wu = nullptr;     // [d_user][dc_dp]: the user rows of Wc_0 in the operand precision, columns in the kernel's order
    float* dc_bc = nullptr;     // [n_cross][dc_dp]: the cross biases in that order
    void* dc_rec = nullptr;     // every matrix as records of one 32-wide input block each, in MFMA fragment order
    // PG_MODEL_MHA (rank_mha.hip; pack_mha below): mh_heads heads over mh_datt attention columns; the trunk's members are a DNN3's
    // whose item half is the 128 rows [e | pooled] of w1, as a DIN's
    uint32_t mh_datt = 0, mh_heads = 0;
    void* mh_wq = nullptr;      // Wq [64][d_att] in MFMA fragment order (bf16 or fp32), output columns in mha_row order
    float* mh_bq = nullptr;     // [d_att] in that order
    float* mh_wk = nullptr;     // [64][d_att] fp32, feature order
    float* mh_wv = nullptr;     // [64][d_att] fp32, output columns in mha_row order
    float* mh_bv = nullptr;     // [d_att] in that order
    void* mh_wo = nullptr;      // Wo [d_att][64] in MFMA fragment order, input rows in feature order
    // PG_MODEL_GBDT (rank_gbdt.hip; pack_gbdt below): gb_ntree complete trees of depth gb_depth over gb_nu user + gb_ni item features
    uint32_t gb_nu = 0, gb_ni = 0, gb_ntree = 0, gb_depth = 0, gb_obj = 0;
    float gb_base = 0.f;
    void* gb_forest = nullptr;  // whole chunks of kGbdtChunkBytes, tree records back to back (gbdt_tree_bytes each)
    // PG_MODEL_MIND (mind.hip): n_out = K interests of mi_dout columns after mi_iter routing iterations; d_user and h1 as a DNN3's
    uint32_t mi_dout = 0, mi_iter = 0, mi_norm = 0;
    float* mi_w = nullptr;      // the blob's arrays as they stand, array i at float MindLayout::at[i]
    float* b2 = nullptr;
    float* w3 = nullptr;    // DNN3 head(s): [n_out][h2]
    float* fields = nullptr;          // two-tower: all field tables, one allocation
    const float** d_field_emb = nullptr;
    const float** d_field_lin = nullptr;
    std::vector<void*> allocs;
};

namespace pg {

constexpr int kDIN = 128;      // gathered input width
constexpr int kMaxHeads = 8;   // outputs of a multi-head DNN3
constexpr int kDinD = 64;      // PG_MODEL_DIN: item width (the trunk's gathered input is [e | pooled] = kDIN)
// PG_PREC_F16X2 / PG_PREC_F16 (the scaling rule is in rank_2r.hip's header)
constexpr int kH2G = 11;       // activations: 2^G on top of the row normalisation
constexpr int kH2S = 23;       // accumulators hold 2^S x the pre-activation; weights carry 2^(S - G)

// (h1, h2) of DNN3 and (t_h1, t_out, k) of the two-tower model; d_item is 64 or 128 (64: the gathered row is padded
// with zero columns whose W1 rows are zero), n_item_fields x k = 128, n_user_fields <= 16
#define PG_DNN3_SHAPES(X) X(128, 128) X(256, 128) X(256, 256) X(512, 256) X(1024, 512)
#define PG_FM2T_SHAPES(X) X(256, 64, 16) X(256, 64, 32) X(128, 64, 8) X(512, 128, 16)
inline bool dnn3_shape_ok(uint32_t h1, uint32_t h2) {
#define X(A, B) if (h1 == A && h2 == B) return true;
    PG_DNN3_SHAPES(X)
#undef X
    return false;
}
// (n_expert, h_e) of an MMoE: E h_e = 256 or 512 layer-1 rows
#define PG_MMOE_SHAPES(X) X(2, 128) X(4, 64) X(4, 128) X(8, 64)
inline bool mmoe_shape_ok(uint32_t ne, uint32_t he) {
#define X(A, B) if (ne == A && he == B) return true;
    PG_MMOE_SHAPES(X)
#undef X
    return false;
}
// PG_MODEL_PLE: T task groups of E_t experts and a shared group of E_s, in one or two extraction levels
inline bool ple_shape_ok(uint32_t du, uint32_t di, uint32_t T, uint32_t et, uint32_t es, uint32_t he, uint32_t nl, uint32_t ht) {
    return (di == 64 || di == 128) && du >= 1 && du <= 4096 && T >= 1 && T <= 3 && (et == 1 || et == 2) && (es == 1 || es == 2) &&
           (nl == 1 || nl == 2) && (he == 64 || (he == 128 && nl == 1)) && (ht == 32 || ht == 64) && (T * et + es) * he <= 512;
}
// PG_MODEL_DCN: D = d_user + d_item is padded to one of these widths (zero rows and columns: a zero coordinate of x_0 stays zero
// through every cross layer); the head is a DNN3's 128-128 or 256-128
constexpr uint32_t dcn_padded(uint32_t d) { return d <= 128 ? 128 : (d <= 192 ? 192 : 256); }
inline bool dcn_shape_ok(uint32_t du, uint32_t di, uint32_t L, uint32_t h1, uint32_t h2, uint32_t n_out) {
    return (di == 64 || di == 128) && du >= 1 && du + di <= 256 && L >= 1 && L <= 3 && (h1 == 128 || h1 == 256) && h2 == 128 && n_out >= 1 &&
           n_out <= 4;
}
// (d_att, n_head) of a PG_MODEL_MHA: head widths 32 and 64
#define PG_MHA_SHAPES(X) X(64, 1) X(64, 2) X(128, 2) X(128, 4)
inline bool mha_shape_ok(uint32_t datt, uint32_t heads) {
#define X(A, B) if (datt == A && heads == B) return true;
    PG_MHA_SHAPES(X)
#undef X
    return false;
}
// PG_MODEL_GBDT: the forest streams through LDS in chunks of whole trees.  A tree's record is 2^d node slots of 8 bytes (slot
// 2^d - 1 unused) and 2^d leaves: 12 << d bytes, so a chunk holds 2^(11 - d) trees exactly — 8 at depth 8, 1024 at depth 1.
constexpr uint32_t kGbdtChunkBytes = PG_GBDT_CHUNK_BYTES;
constexpr uint32_t kGbdtMaxFeat = 64, kGbdtMaxTrees = 4096, kGbdtMaxDepth = 8;
// candidates per workgroup tile: one wave, or four in a call of at least PG_GBDT_WIDE_ITEMS candidates whose feature rows leave
// the two chunk buffers room (kGbdtWideMaxFeat rows of 1 KiB beside 48 KiB)
constexpr uint32_t kGbdtTile = 64, kGbdtWideTile = PG_GBDT_WIDE_TILE, kGbdtWideItems = PG_GBDT_WIDE_ITEMS, kGbdtWideMaxFeat = 80;
constexpr uint32_t gbdt_tree_bytes(uint32_t depth) { return 12u << depth; }
constexpr uint32_t gbdt_chunk_trees(uint32_t depth) { return kGbdtChunkBytes / gbdt_tree_bytes(depth); }
inline bool gbdt_shape_ok(uint32_t nu, uint32_t ni, uint32_t nt, uint32_t d, uint32_t obj) {
    return nu <= kGbdtMaxFeat && ni <= kGbdtMaxFeat && nu + ni >= 1 && nt >= 1 && nt <= kGbdtMaxTrees && d >= 1 && d <= kGbdtMaxDepth && obj <= 1;
}
// PG_MODEL_MIND: where the blob's arrays S, b0, Wc, Wu, b1, W2, b2 start, in floats behind the 24-byte header, and their sum
constexpr uint32_t kMindSeq = PG_MIND_MAX_SEQ, kMindD = 64, kMindMaxK = 8;
enum { kMindS, kMindB0, kMindWc, kMindWu, kMindB1, kMindW2, kMindB2, kMindArrays };
struct MindLayout {
    size_t at[kMindArrays], floats;
    MindLayout(uint32_t d_user, uint32_t d_out, uint32_t K, uint32_t h1) {
        const size_t n[kMindArrays] = {(size_t)kMindD * kMindD, (size_t)K * kMindSeq, (size_t)kMindD * h1, (size_t)d_user * h1, h1, (size_t)h1 * d_out, d_out};
        floats = 0;
        for (int i = 0; i < kMindArrays; ++i) {
            at[i] = floats;
            floats += n[i];
        }
    }
};
inline bool mind_shape_ok(uint32_t du, uint32_t dout, uint32_t K, uint32_t it, uint32_t h1, uint32_t norm) {
    return du >= 1 && du <= 1024 && (dout == 64 || dout == 128) && K >= 1 && K <= kMindMaxK && it >= 1 && it <= 4 && (h1 == 128 || h1 == 256) && norm <= 1;
}
inline bool fm2t_shape_ok(uint32_t th, uint32_t to, uint32_t k) {
#define X(A, B, C) if (th == A && to == B && k == C) return true;
    PG_FM2T_SHAPES(X)
#undef X
    return false;
}

PG_HOST_DEVICE uint16_t f32_to_bf16_rne(float x) {
    uint32_t b;
#ifdef __HIP_DEVICE_COMPILE__
    b = __float_as_uint(x);
#else
    memcpy(&b, &x, 4);
#endif
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((b >> 16) | 0x0040u);
    b += 0x7FFFu + ((b >> 16) & 1u);
    return (uint16_t)(b >> 16);
}
PG_HOST_DEVICE float bf16_to_f32(uint16_t v) {
    uint32_t b = (uint32_t)v << 16;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(b);
#else
    float f;
    memcpy(&f, &b, 4);
    return f;
#endif
}
// operand rounding of a precision mode: 0 = fp32, 1 = bf16 (RNE), 2 = split bf16 (x = hi + lo, three MFMA products:
// nothing is rounded on the scalar side — the mode's specification is the fp32 one)
PG_HOST_DEVICE float round_prec(float x, int prec) {
    return prec == 1 ? bf16_to_f32(f32_to_bf16_rne(x)) : x;
}

// fp32 <-> fp16 (RNE, subnormals kept, NaN quieted) in integer arithmetic: the conversion a _Float16 cast makes, for host
// compilers without the type
inline uint16_t f32_to_f16_rne(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    const uint16_t sign = (uint16_t)((b >> 16) & 0x8000u);
    b &= 0x7FFFFFFFu;
    if (b > 0x7F800000u) return (uint16_t)(sign | 0x7E00u | ((b >> 13) & 0x3FFu));
    if (b >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);              // 65536 and above, infinity
    if (b < 0x38800000u) {                                                // below 2^-14: a multiple of 2^-24
        const uint32_t e = b >> 23;
        if (e < 102) return sign;
        const uint32_t mant = (b & 0x7FFFFFu) | 0x800000u, shift = 126 - e, half = 1u << (shift - 1);
        uint32_t q = mant >> shift;
        const uint32_t rem = mant & ((1u << shift) - 1);
        if (rem > half || (rem == half && (q & 1u))) ++q;
        return (uint16_t)(sign | q);
    }
    b -= 0x38000000u;                                                     // exponent bias 127 -> 15
    b += 0xFFFu + ((b >> 13) & 1u);                                       // (a carry out of [65520, 65536) makes infinity)
    return (uint16_t)(sign | (b >> 13));
}
inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, mant = h & 0x3FFu;
    uint32_t b;
    float f;
    if (e == 0) {
        f = (float)mant * 5.9604644775390625e-8f;                         // x 2^-24, exact
        memcpy(&b, &f, 4);
        b |= sign;
    } else {
        b = sign | ((e == 31 ? 255u : e + 112u) << 23) | (mant << 13);
    }
    memcpy(&f, &b, 4);
    return f;
}

// ---- a refusal: the status pg_model_load returns and the text it reports -------------------------------------------------
struct ModelRefusal {
    int status = PG_OK;
    char text[512] = "";
};
__attribute__((format(printf, 3, 4))) inline int refuse(ModelRefusal* why, int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why->text, sizeof why->text, fmt, ap);
    va_end(ap);
    return why->status = status;
}

// ---- parsing -------------------------------------------------------------------------------------------------------------
// byte offsets of a blob's arrays (fp32, in blob order)
struct BlobLayout {
    // DNN3: W1 [d_user + d_item][h1], b1 [h1], W2 [h1][h2], b2 [h2], W3 [h2][n_out] as exported ([in][out]), b3 [n_out]
    size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0, w3 = 0, b3 = 0;
    // two-tower: the user tower, the item tower, then per field [vocab][k] embeddings and [vocab] linear weights
    size_t uw1 = 0, ub1 = 0, uw2 = 0, ub2 = 0, iw1 = 0, ib1 = 0, iw2 = 0, ib2 = 0, fields = 0;
    size_t field_floats = 0;      // floats of all field tables together
    // DIN, in front of the DNN3 arrays: Wa [4 x 64][att_h] (row blocks e, s, e - s, e * s), ba [att_h], wa2 [att_h], ba2
    size_t wa = 0, ba = 0, wa2 = 0, ba2 = 0;
    // MMoE: We [E][d_user + d_item][h_e], be [E][h_e], Wg [T][d_user + d_item][E], bg [T][E], Wt [T][h_e][h_t], bt [T][h_t],
    // wo [T][h_t], bo [T]
    size_t we = 0, be = 0, wg = 0, bg = 0, wt = 0, bt = 0, wo = 0, bo = 0;
    // DCN, in front of the DNN3 arrays (w1 is [d_user + d_item][h1]): Wc [L][D][D], bc [L][D]
    size_t wc = 0, bc = 0;
    // MHA, in front of the DNN3 arrays: Wq [64][d_att], bq [d_att], Wk [64][d_att], Wv [64][d_att], bv [d_att], Wo [d_att][64]
    size_t a_wq = 0, a_bq = 0, a_wk = 0, a_wv = 0, a_bv = 0, a_wo = 0;
    // PLE, per level l (in = d_user + d_item at level 1, h_e at level 2): We_t [T][E_t][in][h_e], We_s [E_s][in][h_e], be_t [T][E_t][h_e],
    // be_s [E_s][h_e], Wg_t [T][in][E_t + E_s], bg_t [T][E_t + E_s] and, below the last level only, Wg_s [in][T E_t + E_s],
    // bg_s [T E_t + E_s]; then wt, bt, wo, bo as an MMoE's
    size_t ple[2][8] = {};
    // GBDT: tree t at gb_trees + t * gb_tree_bytes: u32 node[2^d - 1], f32 thr[2^d - 1], f32 leaf[2^d]
    size_t gb_trees = 0, gb_tree_bytes = 0;
};
enum { kPleWeT, kPleWeS, kPleBeT, kPleBeS, kPleWgT, kPleBgT, kPleWgS, kPleBgS };

// What `blob` says as a model of `kind` in `prec`: the dimensions (and kind, prec, f16_nprod, b3, fm_b) into *m, the arrays'
// offsets into *lay.  PG_OK, or the refusal in *why.
inline int parse_model_blob(int kind, int prec, const void* blob, size_t len, pg_model* m, BlobLayout* lay, ModelRefusal* why) {
    if (!(prec == PG_PREC_F32 || prec == PG_PREC_BF16 || prec == PG_PREC_BF16X3 || prec == PG_PREC_F16X2 || prec == PG_PREC_F16))
        return refuse(why, PG_ERR_INVALID, "pg_model_load: bad precision %d", prec);
    const int f16_nprod = prec == PG_PREC_F16X2 ? 2 : (prec == PG_PREC_F16 ? 1 : 0);
    if (f16_nprod && kind == PG_MODEL_FM_TWOTOWER)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: PG_PREC_F16X2 / PG_PREC_F16 serve PG_MODEL_DNN3 and PG_MODEL_DNN3_MULTI; load a "
                                               "PG_MODEL_FM_TWOTOWER in PG_PREC_BF16X3");
    if (f16_nprod && kind == PG_MODEL_DIN)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: PG_PREC_F16X2 / PG_PREC_F16 serve PG_MODEL_DNN3 and PG_MODEL_DNN3_MULTI; load a "
                                               "PG_MODEL_DIN in PG_PREC_F32, PG_PREC_BF16 or PG_PREC_BF16X3");
    if (f16_nprod && kind == PG_MODEL_MHA)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: PG_PREC_F16X2 / PG_PREC_F16 serve PG_MODEL_DNN3 and PG_MODEL_DNN3_MULTI; load a "
                                               "PG_MODEL_MHA in PG_PREC_F32, PG_PREC_BF16 or PG_PREC_BF16X3");
    if (kind == PG_MODEL_MMOE && prec != PG_PREC_BF16 && prec != PG_PREC_BF16X3)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a PG_MODEL_MMOE is served in PG_PREC_BF16 and PG_PREC_BF16X3 (precision %d asked)", prec);
    if (kind == PG_MODEL_PLE && prec != PG_PREC_BF16 && prec != PG_PREC_BF16X3)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a PG_MODEL_PLE is served in PG_PREC_BF16 and PG_PREC_BF16X3 (precision %d asked)", prec);
    if (kind == PG_MODEL_GBDT && prec != PG_PREC_F32)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a PG_MODEL_GBDT is served in PG_PREC_F32 (precision %d asked)", prec);
    if (kind == PG_MODEL_DCN && prec != PG_PREC_BF16 && prec != PG_PREC_BF16X3)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a PG_MODEL_DCN is served in PG_PREC_BF16 and PG_PREC_BF16X3 (precision %d asked)", prec);
    if (kind == PG_MODEL_MIND && prec != PG_PREC_F32)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a PG_MODEL_MIND is served in PG_PREC_F32 (precision %d asked)", prec);
    const uint8_t* p = (const uint8_t*)blob;
    // an fp16 mode is the split-bf16 model (its whole-call and per-tile fallback) plus the fp16 operands
    m->prec = f16_nprod ? (int)PG_PREC_BF16X3 : prec;
    m->f16_nprod = f16_nprod;
    if (kind == PG_MODEL_DNN3 || kind == PG_MODEL_DNN3_MULTI) {
        const size_t hb = kind == PG_MODEL_DNN3_MULTI ? 20 : 16;
        m->kind = PG_MODEL_DNN3;                 // every rank entry point takes it; n_out says how many planes it writes
        if (len < hb) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[5] = {0, 0, 0, 0, 1};
        memcpy(hdr, p, hb);
        m->d_user = hdr[0]; m->d_item = hdr[1]; m->h1 = hdr[2]; m->h2 = hdr[3]; m->n_out = hdr[4];
        if (m->n_out == 0 || m->n_out > (uint32_t)kMaxHeads)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a multi-output DNN3 has 1..%d outputs, the blob says %u", kMaxHeads, m->n_out);
        if ((m->d_item != 128 && m->d_item != 64) || !dnn3_shape_ok(m->h1, m->h2) || m->d_user == 0 || m->d_user > 4096)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: DNN3 shape [%u+%u]->%u->%u->1 unsupported (d_item 64 or 128; hidden widths "
                                                   "128-128, 256-128, 256-256, 512-256, 1024-512)", m->d_user, m->d_item, m->h1, m->h2);
        const size_t din = (size_t)m->d_user + m->d_item;
        const size_t need = hb + (din * m->h1 + m->h1 + (size_t)m->h1 * m->h2 + m->h2 + ((size_t)m->h2 + 1) * m->n_out) * 4;
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: DNN3 blob is %zu bytes, expected %zu", len, need);
        lay->w1 = hb;
        lay->b1 = lay->w1 + din * m->h1 * 4;
        lay->w2 = lay->b1 + (size_t)m->h1 * 4;
        lay->b2 = lay->w2 + (size_t)m->h1 * m->h2 * 4;
        lay->w3 = lay->b2 + (size_t)m->h2 * 4;
        lay->b3 = lay->w3 + (size_t)m->h2 * m->n_out * 4;
        memcpy(&m->b3, p + lay->b3, 4);
        if (f16_nprod) {
            const float* w = (const float*)(p + hb);
            for (size_t i = 0; i < (len - hb) / 4; ++i)
                if (!std::isfinite(w[i]))
                    return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: the blob holds a non-finite weight (float %zu): not representable in an fp16 mode", i);
        }
    } else if (kind == PG_MODEL_DIN) {
        m->kind = PG_MODEL_DIN;
        if (len < 24) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[6];
        memcpy(hdr, p, 24);
        m->d_user = hdr[0]; m->d_item = hdr[1]; m->h1 = hdr[2]; m->h2 = hdr[3]; m->n_out = hdr[4]; m->att_h = hdr[5];
        if (m->n_out == 0 || m->n_out > (uint32_t)kMaxHeads)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: a DIN has 1..%d outputs, the blob says %u", kMaxHeads, m->n_out);
        if (m->d_item != (uint32_t)kDinD || (m->att_h != 16 && m->att_h != 32) || !dnn3_shape_ok(m->h1, m->h2) || m->d_user == 0 ||
            m->d_user > 4096)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: DIN shape [%u+2x%u]->%u->%u, attention width %u unsupported (d_item 64; "
                                                   "attention width 16 or 32; hidden widths 128-128, 256-128, 256-256, 512-256, 1024-512)",
                          m->d_user, m->d_item, m->h1, m->h2, m->att_h);
        const size_t att = (size_t)4 * kDinD * m->att_h + 2 * m->att_h + 1, din = (size_t)m->d_user + 2 * kDinD;
        const size_t need = 24 + (att + din * m->h1 + m->h1 + (size_t)m->h1 * m->h2 + m->h2 + ((size_t)m->h2 + 1) * m->n_out) * 4;
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: DIN blob is %zu bytes, expected %zu", len, need);
        lay->wa = 24;
        lay->ba = lay->wa + (size_t)4 * kDinD * m->att_h * 4;
        lay->wa2 = lay->ba + (size_t)m->att_h * 4;
        lay->ba2 = lay->wa2 + (size_t)m->att_h * 4;
        lay->w1 = lay->ba2 + 4;
        lay->b1 = lay->w1 + din * m->h1 * 4;
        lay->w2 = lay->b1 + (size_t)m->h1 * 4;
        lay->b2 = lay->w2 + (size_t)m->h1 * m->h2 * 4;
        lay->w3 = lay->b2 + (size_t)m->h2 * 4;
        lay->b3 = lay->w3 + (size_t)m->h2 * m->n_out * 4;
        memcpy(&m->att_ba2, p + lay->ba2, 4);
        memcpy(&m->b3, p + lay->b3, 4);
    } else if (kind == PG_MODEL_MHA) {
        m->kind = PG_MODEL_MHA;
        if (len < 28) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[7];
        memcpy(hdr, p, 28);
        m->d_user = hdr[0]; m->d_item = hdr[1]; m->h1 = hdr[2]; m->h2 = hdr[3]; m->n_out = hdr[4]; m->mh_datt = hdr[5]; m->mh_heads = hdr[6];
        if (m->n_out == 0 || m->n_out > (uint32_t)kMaxHeads)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: an MHA has 1..%d outputs, the blob says %u", kMaxHeads, m->n_out);
        if (m->d_item != (uint32_t)kDinD || !mha_shape_ok(m->mh_datt, m->mh_heads) || !dnn3_shape_ok(m->h1, m->h2) || m->d_user == 0 ||
            m->d_user > 4096)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: MHA shape [%u+2x%u]->%u->%u, d_att %u in %u heads unsupported (d_item 64; (d_att, heads) "
                                                   "(64,1) (64,2) (128,2) (128,4); hidden widths 128-128, 256-128, 256-256, 512-256, 1024-512)",
                          m->d_user, m->d_item, m->h1, m->h2, m->mh_datt, m->mh_heads);
        const size_t da = m->mh_datt, din = (size_t)m->d_user + 2 * kDinD;
        const size_t nf[12] = {kDinD * da, da, kDinD * da, kDinD * da, da, da * kDinD, din * m->h1, m->h1, (size_t)m->h1 * m->h2, m->h2,
                               (size_t)m->h2 * m->n_out, m->n_out};
        size_t* const at[12] = {&lay->a_wq, &lay->a_bq, &lay->a_wk, &lay->a_wv, &lay->a_bv, &lay->a_wo, &lay->w1, &lay->b1, &lay->w2, &lay->b2, &lay->w3, &lay->b3};
        size_t need = 28;
        for (int i = 0; i < 12; ++i) {
            *at[i] = need;
            need += nf[i] * 4;
        }
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: MHA blob is %zu bytes, expected %zu", len, need);
        memcpy(&m->b3, p + lay->b3, 4);
    } else if (kind == PG_MODEL_MMOE) {
        m->kind = PG_MODEL_MMOE;
        if (len < 24) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[6];
        memcpy(hdr, p, 24);
        m->d_user = hdr[0]; m->d_item = hdr[1]; m->n_expert = hdr[2]; m->h_e = hdr[3]; m->n_out = hdr[4]; m->h_t = hdr[5];
        if ((m->d_item != 128 && m->d_item != 64) || !mmoe_shape_ok(m->n_expert, m->h_e) || m->n_out == 0 || m->n_out > 4 ||
            (m->h_t != 32 && m->h_t != 64) || m->d_user == 0 || m->d_user > 4096)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: MMoE shape [%u+%u] -> %u experts x %u -> %u towers x %u unsupported (d_item 64 or "
                                                   "128; experts x width 2x128, 4x64, 4x128, 8x64; 1..4 tasks; tower width 32 or 64)",
                          m->d_user, m->d_item, m->n_expert, m->h_e, m->n_out, m->h_t);
        m->mm_tp = m->n_out <= 2 ? 2 : 4;
        const size_t din = (size_t)m->d_user + m->d_item, E = m->n_expert, he = m->h_e, T = m->n_out, ht = m->h_t;
        const size_t nf[8] = {E * din * he, E * he, T * din * E, T * E, T * he * ht, T * ht, T * ht, T};
        size_t* const at[8] = {&lay->we, &lay->be, &lay->wg, &lay->bg, &lay->wt, &lay->bt, &lay->wo, &lay->bo};
        size_t need = 24;
        for (int i = 0; i < 8; ++i) {
            *at[i] = need;
            need += nf[i] * 4;
        }
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: MMoE blob is %zu bytes, expected %zu", len, need);
    } else if (kind == PG_MODEL_PLE) {
        m->kind = PG_MODEL_PLE;
        if (len < 32) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[8];
        memcpy(hdr, p, 32);
        m->d_user = hdr[0]; m->d_item = hdr[1]; m->n_out = hdr[2]; m->e_task = hdr[3]; m->e_shared = hdr[4]; m->h_e = hdr[5]; m->n_level = hdr[6];
        m->h_t = hdr[7];
        if (!ple_shape_ok(m->d_user, m->d_item, m->n_out, m->e_task, m->e_shared, m->h_e, m->n_level, m->h_t))
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: PLE shape [%u+%u] -> %u levels of %u x %u task and %u shared experts x %u -> towers x %u "
                                                   "unsupported (d_item 64 or 128; 1..3 tasks; 1 or 2 experts per group; width 64, or 128 with one level; "
                                                   "1 or 2 levels; tower width 32 or 64; all experts x width <= 512)",
                          m->d_user, m->d_item, m->n_level, m->n_out, m->e_task, m->e_shared, m->h_e, m->h_t);
        m->pl_nrec1 = (m->h_e / 16) * (m->n_out + 1);
        const size_t T = m->n_out, Et = m->e_task, Es = m->e_shared, he = m->h_e, ht = m->h_t;
        size_t need = 32;
        for (uint32_t l = 0; l < m->n_level; ++l) {
            const size_t in = l ? he : (size_t)m->d_user + m->d_item, last = l + 1 == m->n_level;
            const size_t nf[8] = {T * Et * in * he, Es * in * he, T * Et * he, Es * he, T * in * (Et + Es), T * (Et + Es),
                                  last ? 0 : in * (T * Et + Es), last ? 0 : T * Et + Es};
            for (int i = 0; i < 8; ++i) {
                lay->ple[l][i] = need;
                need += nf[i] * 4;
            }
        }
        const size_t nf[4] = {T * he * ht, T * ht, T * ht, T};
        size_t* const at[4] = {&lay->wt, &lay->bt, &lay->wo, &lay->bo};
        for (int i = 0; i < 4; ++i) {
            *at[i] = need;
            need += nf[i] * 4;
        }
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: PLE blob is %zu bytes, expected %zu", len, need);
    } else if (kind == PG_MODEL_GBDT) {
        m->kind = PG_MODEL_GBDT;
        if (len < 24) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[5];
        memcpy(hdr, p, 20);
        memcpy(&m->gb_base, p + 20, 4);
        m->gb_nu = hdr[0]; m->gb_ni = hdr[1]; m->gb_ntree = hdr[2]; m->gb_depth = hdr[3]; m->gb_obj = hdr[4];
        m->n_out = 1;
        if (!gbdt_shape_ok(m->gb_nu, m->gb_ni, m->gb_ntree, m->gb_depth, m->gb_obj))
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: GBDT shape [%u+%u] features, %u trees of depth %u, objective %u unsupported (0..64 "
                                                   "user and 0..64 item features, at least one; 1..4096 trees; depth 1..8; objective 0 or 1)",
                          m->gb_nu, m->gb_ni, m->gb_ntree, m->gb_depth, m->gb_obj);
        const size_t nn = ((size_t)1 << m->gb_depth) - 1, nl = nn + 1;
        lay->gb_trees = 24;
        lay->gb_tree_bytes = (2 * nn + nl) * 4;
        const size_t need = 24 + m->gb_ntree * lay->gb_tree_bytes;
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: GBDT blob is %zu bytes, expected %zu", len, need);
        if (!std::isfinite(m->gb_base)) return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: the GBDT's base score is not finite");
        for (uint32_t t = 0; t < m->gb_ntree; ++t) {
            const uint8_t* const tr = p + lay->gb_trees + t * lay->gb_tree_bytes;
            for (size_t n = 0; n < nn; ++n) {
                uint32_t w;
                float thr;
                memcpy(&w, tr + n * 4, 4);
                memcpy(&thr, tr + (nn + n) * 4, 4);
                if ((w & 0x7Fu) >= m->gb_nu + m->gb_ni)
                    return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: GBDT tree %u node %zu splits on feature %u of %u", t, n, w & 0x7Fu, m->gb_nu + m->gb_ni);
                if (thr != thr) return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: GBDT tree %u node %zu has a NaN threshold", t, n);
            }
            for (size_t l = 0; l < nl; ++l) {
                float v;
                memcpy(&v, tr + (2 * nn + l) * 4, 4);
                if (!std::isfinite(v)) return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: GBDT tree %u leaf %zu is not finite", t, l);
            }
        }
    } else if (kind == PG_MODEL_MIND) {
        m->kind = PG_MODEL_MIND;
        if (len < 24) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[6];
        memcpy(hdr, p, 24);
        m->d_user = hdr[0]; m->mi_dout = hdr[1]; m->n_out = hdr[2]; m->mi_iter = hdr[3]; m->h1 = hdr[4]; m->mi_norm = hdr[5];
        if (!mind_shape_ok(m->d_user, m->mi_dout, m->n_out, m->mi_iter, m->h1, m->mi_norm))
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: MIND shape d_user %u, d_out %u, %u interests, %u iterations, h1 %u, normalize %u "
                                                   "unsupported (d_user 1..1024; d_out 64 or 128; 1..8 interests; 1..4 iterations; h1 128 or 256; "
                                                   "normalize 0 or 1)", m->d_user, m->mi_dout, m->n_out, m->mi_iter, m->h1, m->mi_norm);
        const size_t nfl = MindLayout(m->d_user, m->mi_dout, m->n_out, m->h1).floats;
        if (len != 24 + nfl * 4) return refuse(why, PG_ERR_INVALID, "pg_model_load: MIND blob is %zu bytes, expected %zu", len, 24 + nfl * 4);
        for (size_t i = 0; i < nfl; ++i) {
            float v;
            memcpy(&v, p + 24 + i * 4, 4);
            if (!std::isfinite(v)) return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: the MIND blob holds a non-finite weight (float %zu)", i);
        }
    } else if (kind == PG_MODEL_DCN) {
        m->kind = PG_MODEL_DCN;
        if (len < 24) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[6];
        memcpy(hdr, p, 24);
        m->d_user = hdr[0]; m->d_item = hdr[1]; m->n_cross = hdr[2]; m->h1 = hdr[3]; m->h2 = hdr[4]; m->n_out = hdr[5];
        if (!dcn_shape_ok(m->d_user, m->d_item, m->n_cross, m->h1, m->h2, m->n_out))
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: DCN shape [%u+%u], %u cross layers -> %u -> %u -> %u outputs unsupported (d_item 64 "
                                                   "or 128; d_user + d_item <= 256; 1..3 cross layers; hidden widths 128-128, 256-128; 1..4 outputs)",
                          m->d_user, m->d_item, m->n_cross, m->h1, m->h2, m->n_out);
        m->dc_dp = dcn_padded(m->d_user + m->d_item);
        const size_t D = (size_t)m->d_user + m->d_item, L = m->n_cross;
        const size_t nf[8] = {L * D * D, L * D, D * m->h1, m->h1, (size_t)m->h1 * m->h2, m->h2, (size_t)m->h2 * m->n_out, m->n_out};
        size_t* const at[8] = {&lay->wc, &lay->bc, &lay->w1, &lay->b1, &lay->w2, &lay->b2, &lay->w3, &lay->b3};
        size_t need = 24;
        for (int i = 0; i < 8; ++i) {
            *at[i] = need;
            need += nf[i] * 4;
        }
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: DCN blob is %zu bytes, expected %zu", len, need);
        memcpy(&m->b3, p + lay->b3, 4);
    } else if (kind == PG_MODEL_FM_TWOTOWER) {
        m->kind = PG_MODEL_FM_TWOTOWER;
        if (len < 32) return refuse(why, PG_ERR_INVALID, "pg_model_load: blob too short");
        uint32_t hdr[7];
        memcpy(hdr, p, 28);
        memcpy(&m->fm_b, p + 28, 4);
        m->nuf = hdr[0]; m->nif = hdr[1]; m->k = hdr[2]; m->d_user = hdr[3];
        m->th = hdr[4]; m->to = hdr[5]; m->vocab = hdr[6];
        // (the product in 64 bits: 0x10000008 fields x 16 is not 128)
        if (m->nuf == 0 || m->nuf > 16 || (uint64_t)m->nif * m->k != (uint64_t)kDIN || !fm2t_shape_ok(m->th, m->to, m->k) ||
            m->d_user == 0 || m->d_user > 4096 || m->vocab == 0)
            return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: two-tower shape unsupported (1..16 user fields; item fields x k = 128 with "
                                                   "k = 8, 16 or 32; towers 256-64 (k 16 / 32), 128-64 (k 8), 512-128 (k 16))");
        const size_t din = (size_t)m->nif * m->k;
        const size_t nf = m->nuf + m->nif;
        const size_t wfl = (size_t)m->d_user * m->th + m->th + (size_t)m->th * m->to + m->to + din * m->th +
                           m->th + (size_t)m->th * m->to + m->to;
        lay->field_floats = nf * ((size_t)m->vocab * m->k + m->vocab);
        const size_t need = 32 + (wfl + lay->field_floats) * 4;
        if (len != need) return refuse(why, PG_ERR_INVALID, "pg_model_load: two-tower blob is %zu bytes, expected %zu", len, need);
        lay->uw1 = 32;
        lay->ub1 = lay->uw1 + (size_t)m->d_user * m->th * 4;
        lay->uw2 = lay->ub1 + (size_t)m->th * 4;
        lay->ub2 = lay->uw2 + (size_t)m->th * m->to * 4;
        lay->iw1 = lay->ub2 + (size_t)m->to * 4;
        lay->ib1 = lay->iw1 + din * m->th * 4;
        lay->iw2 = lay->ib1 + (size_t)m->th * 4;
        lay->ib2 = lay->iw2 + (size_t)m->th * m->to * 4;
        lay->fields = lay->ib2 + (size_t)m->to * 4;
    } else {
        return refuse(why, PG_ERR_INVALID, "pg_model_load: unknown model kind %d", kind);
    }
    return PG_OK;
}

// ---- packing -------------------------------------------------------------------------------------------------------------
// Pack W[K][N] (row-major, k major) into MFMA B-fragment order, 1 KiB per (n-block, k-group).
//   bf16: fragment (nbg, ks): lane (j,hk) holds W[ks*16 + 8*hk + e][nbg*32 + j], e = 0..7
//   f32 : fragment (nbg, g8): lane (j,h)  holds W[g8*8 + 2*st + h][nbg*32 + j], st = 0..3
//   split bf16 (prec 2): the bf16 layout twice — every hi fragment, then every lo fragment (lo = RNE(w - hi))
inline std::vector<uint8_t> pack_weights(const float* w, uint32_t K, uint32_t N, int prec) {
    const uint32_t kg = prec ? K / 16 : K / 8;
    const size_t plane = (size_t)(N / 32) * kg * 1024;
    std::vector<uint8_t> out(plane * (prec == 2 ? 2 : 1));
    for (uint32_t nbg = 0; nbg < N / 32; ++nbg)
        for (uint32_t g = 0; g < kg; ++g) {
            uint8_t* frag = out.data() + ((size_t)nbg * kg + g) * 1024;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t j = lane & 31, hh = lane >> 5;
                if (prec) {
                    uint16_t* d = reinterpret_cast<uint16_t*>(frag + lane * 16);
                    uint16_t* dl = reinterpret_cast<uint16_t*>(frag + plane + lane * 16);
                    for (uint32_t e = 0; e < 8; ++e) {
                        const float v = w[(size_t)(g * 16 + 8 * hh + e) * N + nbg * 32 + j];
                        d[e] = f32_to_bf16_rne(v);
                        if (prec == 2) dl[e] = f32_to_bf16_rne(v - bf16_to_f32(d[e]));
                    }
                } else {
                    float* d = reinterpret_cast<float*>(frag + lane * 16);
                    for (uint32_t st = 0; st < 4; ++st)
                        d[st] = w[(size_t)(g * 8 + 2 * st + hh) * N + nbg * 32 + j];
                }
            }
        }
    return out;
}

// PG_PREC_F16X2 / PG_PREC_F16 (rank_2r.hip): the bf16 fragment layout in fp16 — every hi fragment (RNE), then, with two
// products per term, every lo fragment (lo = RNE(w - hi))
inline std::vector<uint8_t> pack_weights_f16(const float* w, uint32_t K, uint32_t N, int nprod) {
    const uint32_t kg = K / 16;
    const size_t plane = (size_t)(N / 32) * kg * 1024;
    std::vector<uint8_t> out(plane * nprod);
    for (uint32_t nbg = 0; nbg < N / 32; ++nbg)
        for (uint32_t g = 0; g < kg; ++g) {
            uint8_t* frag = out.data() + ((size_t)nbg * kg + g) * 1024;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t j = lane & 31, hh = lane >> 5;
                uint16_t hi[8], lo[8];
                for (uint32_t e = 0; e < 8; ++e) {
                    const float v = w[(size_t)(g * 16 + 8 * hh + e) * N + nbg * 32 + j];
                    hi[e] = f32_to_f16_rne(v);
                    lo[e] = f32_to_f16_rne(v - f16_to_f32(hi[e]));
                }
                memcpy(frag + lane * 16, hi, 16);
                if (nprod == 2) memcpy(frag + plane + lane * 16, lo, 16);
            }
        }
    return out;
}

// floor(log2 max_j |row[j]|), 0 for an all-zero row; false for a non-finite entry
inline bool row_exponent(const float* row, size_t n, int* e) {
    float mx = 0.0f;
    for (size_t j = 0; j < n; ++j) {
        if (!std::isfinite(row[j])) return false;
        mx = std::max(mx, std::fabs(row[j]));
    }
    *e = mx > 0.0f ? std::ilogb(mx) : 0;
    return true;
}

// The fp16 modes' operands (the scaling rule is in rank_2r.hip's header): W1's item half [kDIN][h1] and W2 [h1][h2] scaled
// per row, the activations' factors beside them.  PG_ERR_UNSUPPORTED for weights the rule cannot carry.
inline int build_f16_operands(const float* w1i, const float* w2, uint32_t h1, uint32_t h2, int nprod,
                              std::vector<uint8_t>* w1p, std::vector<uint8_t>* w2p, std::vector<float>* xs,
                              std::vector<float>* hs, ModelRefusal* why) {
    auto scale_rows = [&](const float* w, uint32_t K, uint32_t N, int act_bias, std::vector<float>* ws,
                          std::vector<float>* fs, const char* what) {
        ws->assign((size_t)K * N, 0.0f);
        fs->assign(K, 0.0f);
        for (uint32_t k = 0; k < K; ++k) {
            int e;
            if (!row_exponent(w + (size_t)k * N, N, &e))
                return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: %s row %u holds a non-finite weight: not representable in an fp16 mode", what, k);
            // act_bias: G for x (accumulator scale S comes from the weights), G - S for h1 (whose accumulators carry 2^S)
            const float f = std::ldexp(1.0f, e + act_bias), g = std::ldexp(1.0f, -e - kH2G + kH2S);
            bool ok = std::isnormal(f) && std::isnormal(g);
            for (uint32_t j = 0; j < N && ok; ++j) {
                const float v = w[(size_t)k * N + j] * g;
                // (a weight 2^-100 of its row's maximum may vanish: it is under every bound here)
                ok = std::isfinite(v);
                (*ws)[(size_t)k * N + j] = v;
            }
            if (!ok)
                return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: %s row %u (largest weight 2^%d) leaves fp32's normal range once scaled for an fp16 mode",
                              what, k, e);
            (*fs)[k] = f;
        }
        return (int)PG_OK;
    };
    std::vector<float> w1s, w2s;
    int rc;
    if ((rc = scale_rows(w1i, kDIN, h1, kH2G, &w1s, xs, "W1 (item half)"))) return rc;
    if ((rc = scale_rows(w2, h1, h2, kH2G - kH2S, &w2s, hs, "W2"))) return rc;
    *w1p = pack_weights_f16(w1s.data(), kDIN, h1, nprod);
    *w2p = pack_weights_f16(w2s.data(), h1, h2, nprod);
    return PG_OK;
}

inline std::vector<float> rounded(const float* w, size_t n, int prec) {
    std::vector<float> o(n);
    for (size_t i = 0; i < n; ++i) o[i] = round_prec(w[i], prec);
    return o;
}

// PG_MODEL_DIN: the activation unit's first layer Wa = [We; Ws; Wd; Wp] ([4 x 64][att_h], input [e | s | e - s | e * s]) folded
// so that no per-pair operand is formed:  Wa' z = (We + Wd)' e + (Ws - Wd)' s + Wp' (e * s)  =  Wq' e + Wk' s + Wp' (e * s).
// Each output [64][att_h], fp32 sums of fp32 weights (nothing is rounded here in any precision: rank_din.hip rounds the
// operand it builds from them, once).
inline void fold_din_attention(const float* wa, uint32_t att_h, std::vector<float>* wq, std::vector<float>* wk, std::vector<float>* wp) {
    const size_t n = (size_t)kDinD * att_h;
    const float *we = wa, *ws = wa + n, *wd = wa + 2 * n, *wpp = wa + 3 * n;
    wq->resize(n); wk->resize(n); wp->assign(wpp, wpp + n);
    for (size_t i = 0; i < n; ++i) {
        (*wq)[i] = we[i] + wd[i];
        (*wk)[i] = ws[i] - wd[i];
    }
}

// PG_MODEL_MMOE: where rank_mmoe.hip wants each weight.  Candidates sit on the MFMA column axis, so a lane (item, half hk) holds
// rows p = (r & 3) + 8 (r >> 2) + 4 hk, r = 0..15, of a 32-row accumulator block; mmoe_slot gives (hk, r) of row p.
//   gate block (one):          slot G = 16 hk + r is logit (task G / E, expert G % E), zero rows from task T on: a lane half holds
//                              whole tasks (16 % E = 0)
//   layer 1, step s, block b:  slot q = 16 b + r of the step's 8 E slots per half is (expert q % E, hidden unit 16 s + 8 hk + q / E):
//                              a lane holds all E experts of 8 consecutive hidden units, exactly the 8 k-values it supplies as the
//                              tower product's B operand for the step's 16-deep slice
// Column order of wu / bu (and of a request's c1): the 32 gate rows, then rows (s, b, p) ascending.
inline void mmoe_slot(uint32_t p, uint32_t* hk, uint32_t* r) {
    *hk = (p >> 2) & 1;
    *r = (p & 3) + 4 * (p >> 3);
}
// 8 consecutive k-values of one lane of fragment `frag` of the record at `rec`, in `planes` bf16 planes (hi, then what is left)
inline void frag_put(uint8_t* rec, uint32_t frag, uint32_t lane, const float* v, uint32_t planes) {
    uint16_t* const d = reinterpret_cast<uint16_t*>(rec + (size_t)frag * planes * 1024 + lane * 16);
    for (uint32_t e = 0; e < 8; ++e) {
        float rest = v[e];
        for (uint32_t pl = 0; pl < planes; ++pl) {
            d[512 * pl + e] = f32_to_bf16_rne(rest);
            rest -= bf16_to_f32(d[512 * pl + e]);       // (exact)
        }
    }
}
struct MmoePacked {
    std::vector<float> wu, bu, bt, wo, bo;
    std::vector<uint8_t> rec;
};
// (split bf16: the gate record carries THREE planes — hi, mid, lo = the weight's 24 bits exactly — because a logit is an exponent:
//  two planes leave 2^-18 of a +-80 logit, which the softmax turns into 5e-7 of a score)
constexpr size_t mmoe_gate_bytes(uint32_t d_item, int prec) { return (size_t)(d_item / 16) * (prec == 2 ? 3 : 1) * 1024; }
constexpr size_t mmoe_step_bytes(uint32_t d_item, uint32_t E, uint32_t tp, uint32_t ht, int prec) {
    return ((size_t)(E / 2) * (d_item / 16) + tp * ht / 32) * (prec == 2 ? 2 : 1) * 1024;
}
// Records in fragment order (1 KiB per fragment: lane l's 8 bf16 at 16 l; split bf16: the lo fragment follows its hi fragment, in
// the gate record the mid and the lo fragment):
//   gate record:    fragment ks          lane (p, hk') = Wg row (slot of p), item columns 16 ks + 8 hk' + 0..7
//   step record s:  fragment b KS + ks   lane (p, hk') = We row (s, b, slot of p), the same columns;
//                   then fragment tb = t h_t / 32 + hb: lane (i, hk') = Wt_t[16 s + 8 hk' + 0..7][32 hb + i]
inline void pack_mmoe(const pg_model* m, const float* we, const float* be, const float* wg, const float* bg, const float* wt,
                      const float* bt, const float* wo, const float* bo, MmoePacked* o) {
    const uint32_t du = m->d_user, D = m->d_item, din = du + D, E = m->n_expert, he = m->h_e, T = m->n_out, ht = m->h_t, TP = m->mm_tp;
    const uint32_t KS = D / 16, EB = E / 2, S = he / 16, NC = 32 + E * he, PL = m->prec == 2 ? 2 : 1, HB = ht / 32;
    const size_t gbytes = mmoe_gate_bytes(D, m->prec), sbytes = mmoe_step_bytes(D, E, TP, ht, m->prec);
    o->wu.assign((size_t)du * NC, 0.0f);
    o->bu.assign(NC, 0.0f);
    o->rec.assign(gbytes + S * sbytes, 0);
    o->bt.assign((size_t)TP * ht, 0.0f);
    o->wo.assign((size_t)TP * ht, 0.0f);
    o->bo.assign(TP, 0.0f);
    memcpy(o->bt.data(), bt, (size_t)T * ht * 4);
    memcpy(o->wo.data(), wo, (size_t)T * ht * 4);
    memcpy(o->bo.data(), bo, (size_t)T * 4);
    // one row of the big product: input-major column `col` of W ([din][ncol]) into column `c` of wu / bu and row p of `frag0 + ks`
    auto row = [&](uint8_t* rec, uint32_t frag0, uint32_t planes, uint32_t p, uint32_t c, const float* W, uint32_t ncol, uint32_t col, float bias) {
        for (uint32_t k = 0; k < du; ++k) o->wu[(size_t)k * NC + c] = round_prec(W[(size_t)k * ncol + col], m->prec);
        o->bu[c] = bias;
        for (uint32_t ks = 0; ks < KS; ++ks)
            for (uint32_t hh = 0; hh < 2; ++hh) {
                float v[8];
                for (uint32_t e = 0; e < 8; ++e) v[e] = W[(size_t)(du + ks * 16 + 8 * hh + e) * ncol + col];
                frag_put(rec, frag0 + ks, hh * 32 + p, v, planes);
            }
    };
    for (uint32_t p = 0; p < 32; ++p) {
        uint32_t hk, r;
        mmoe_slot(p, &hk, &r);
        const uint32_t G = 16 * hk + r, t = G / E, k = G % E;
        if (t < T) row(o->rec.data(), 0, PL == 2 ? 3 : 1, p, p, wg + (size_t)t * din * E, E, k, bg[t * E + k]);
        for (uint32_t s = 0; s < S; ++s)
            for (uint32_t b = 0; b < EB; ++b) {
                const uint32_t q = 16 * b + r, x = q % E, j = 16 * s + 8 * hk + q / E;
                row(o->rec.data() + gbytes + s * sbytes, b * KS, PL, p, 32 + (s * EB + b) * 32 + p, we + (size_t)x * din * he, he, j, be[x * he + j]);
            }
    }
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t hb = 0; hb < HB; ++hb)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    float v[8];
                    for (uint32_t e = 0; e < 8; ++e) v[e] = wt[((size_t)t * he + 16 * s + 8 * (lane >> 5) + e) * ht + 32 * hb + (lane & 31)];
                    frag_put(o->rec.data() + gbytes + s * sbytes, EB * KS + t * HB + hb, lane, v, PL);
                }
}

// PG_MODEL_PLE: where rank_ple.hip wants each weight.  Candidates sit on the MFMA column axis as for an MMoE, a lane (item, half hk)
// holding rows p of a 32-row accumulator block in registers r, (hk, r) = mmoe_slot(p).  Group positions: task t at t, the shared
// group at 3, whatever T is.
//   gate block (one, level 1):  half 0, slot r = 4 t + c: task t's logit over its own expert c (c < 2) or shared expert c - 2; half 1,
//                               slot r: the shared gate's logit over task r / 2's expert r % 2 (r < 6) or shared expert r - 6.  Rows
//                               of experts the model does not have stay zero; the kernel masks them (ple_task_mask, ple_shared_mask)
//   an expert block:            slot r = 8 k + u of half hk is (expert k of the group, hidden unit 16 s + 8 hk + u): a lane holds both
//                               experts of 8 consecutive hidden units, the 8 k-values it supplies to the next product's 16-deep slice s
// Records (ple_rec1_bytes each at level 1, ple_rec2_bytes at level 2), in the order the kernel consumes them: level 1, then level 2; in a level step s = 0 .. h_e / 16 - 1;
// in a step the shared group, then task 0 .. T - 1.  A record's fragments (1 KiB each; split bf16: the lo fragment follows its hi):
//   level 1:  fragment ks < d_item / 16: lane (p, hk') = We1 row (slot of p), item columns 16 ks + 8 hk' + 0..7 (split bf16 under a
//             second level: hi, mid and lo fragments, ple_l1_planes)
//   level 2:  fragment ks < 4:           lane (p, hk') = We2 row (slot of p), inputs 16 ks + 8 hk' + 0..7 of the group's x1
//   last level, a task's record:  then fragment hb < h_t / 32: lane (i, hk') = Wt_t[16 s + 8 hk' + 0..7][32 hb + i]
// In front of the records the gate record (as an MMoE's: three planes in split bf16) and, with two levels, the second level's task
// gates for the fp32 chains: float4 [3][64] = Wg2_t[j][own 0, own 1, shared 0, shared 1] in the operand precision.
// Column order of wu / bu (and of a request's c1): the 32 gate rows, then 32 rows per level-1 record.
// (split bf16, two levels: level 1's expert fragments carry THREE planes as the gate record does — level 2's gates exponentiate
//  what those experts produce, and the 2^-18 a two-way split leaves of x1 showed as 3e-7 of a score under +-80 logits)
constexpr uint32_t ple_l1_planes(uint32_t n_level, int prec) { return prec == 2 ? (n_level == 2 ? 3 : 2) : 1; }
constexpr size_t ple_rec1_bytes(uint32_t d_item, uint32_t n_level, uint32_t ht, int prec) {
    return (size_t)(d_item / 16 + (n_level == 1 ? ht / 32 : 0)) * ple_l1_planes(n_level, prec) * 1024;
}
constexpr size_t ple_rec2_bytes(uint32_t ht, int prec) { return (size_t)(4 + ht / 32) * (prec == 2 ? 2 : 1) * 1024; }
constexpr size_t ple_gate_bytes(uint32_t d_item, uint32_t n_level, int prec) {
    return mmoe_gate_bytes(d_item, prec) + (n_level == 2 ? 3 * 64 * 16 : 0);
}
constexpr uint32_t ple_task_mask(uint32_t et, uint32_t es) { return (et == 2 ? 3u : 1u) | (es == 2 ? 12u : 4u); }
constexpr uint32_t ple_shared_mask(uint32_t T, uint32_t et, uint32_t es) {
    uint32_t m = (es == 2 ? 3u : 1u) << 6;
    for (uint32_t t = 0; t < T; ++t) m |= (et == 2 ? 3u : 1u) << (2 * t);
    return m;
}
struct PlePacked {
    std::vector<float> wu, bu, be2, bg2, bt, wo, bo;
    std::vector<uint8_t> rec;
};
inline void pack_ple(const pg_model* m, const uint8_t* blob, const BlobLayout& lay, PlePacked* o) {
    const uint32_t du = m->d_user, D = m->d_item, din = du + D, T = m->n_out, Et = m->e_task, Es = m->e_shared, he = m->h_e, ht = m->h_t;
    const uint32_t NL = m->n_level, KS = D / 16, S = he / 16, HB = ht / 32, PL = m->prec == 2 ? 2 : 1, NR1 = m->pl_nrec1, NC = 32 + 32 * NR1;
    const size_t gfrag = mmoe_gate_bytes(D, m->prec), gbytes = ple_gate_bytes(D, NL, m->prec);
    const size_t rb1 = ple_rec1_bytes(D, NL, ht, m->prec), rb2 = ple_rec2_bytes(ht, m->prec);
    const uint32_t P1 = ple_l1_planes(NL, m->prec);
    auto arr = [&](uint32_t l, int i) { return (const float*)(blob + lay.ple[l][i]); };
    const float* const wt = (const float*)(blob + lay.wt);
    o->wu.assign((size_t)du * NC, 0.0f);
    o->bu.assign(NC, 0.0f);
    o->rec.assign(gbytes + NR1 * (rb1 + (NL == 2 ? rb2 : 0)), 0);
    auto record = [&](uint32_t l, uint32_t ri) { return o->rec.data() + gbytes + (l ? NR1 * rb1 + ri * rb2 : ri * rb1); };
    o->be2.assign(NL == 2 ? (size_t)NR1 * 32 : 32, 0.0f);
    o->bg2.assign(12, 0.0f);
    o->bt.assign((size_t)3 * ht, 0.0f);
    o->wo.assign((size_t)3 * ht, 0.0f);
    o->bo.assign(3, 0.0f);
    memcpy(o->bt.data(), blob + lay.bt, (size_t)T * ht * 4);
    memcpy(o->wo.data(), blob + lay.wo, (size_t)T * ht * 4);
    memcpy(o->bo.data(), blob + lay.bo, (size_t)T * 4);
    // one row of a level-1 product: column `col` of W ([din][ncol]) into column c of wu / bu and row p of fragments frag0 + ks
    auto row1 = [&](uint8_t* rec, uint32_t planes, uint32_t p, uint32_t c, const float* W, uint32_t ncol, uint32_t col, float bias) {
        for (uint32_t k = 0; k < du; ++k) o->wu[(size_t)k * NC + c] = round_prec(W[(size_t)k * ncol + col], m->prec);
        o->bu[c] = bias;
        for (uint32_t ks = 0; ks < KS; ++ks)
            for (uint32_t hh = 0; hh < 2; ++hh) {
                float v[8];
                for (uint32_t e = 0; e < 8; ++e) v[e] = W[(size_t)(du + ks * 16 + 8 * hh + e) * ncol + col];
                frag_put(rec, ks, hh * 32 + p, v, planes);
            }
    };
    // group g's (T: the shared group's) expert k of level l: its matrix [in][h_e] and bias [h_e], or null
    auto expert = [&](uint32_t l, uint32_t g, uint32_t k, const float** W, const float** b) {
        const size_t in = l ? he : din;
        if (k >= (g < T ? Et : Es)) return false;
        const size_t x = g < T ? (size_t)g * Et + k : k;
        *W = arr(l, g < T ? kPleWeT : kPleWeS) + x * in * he;
        *b = arr(l, g < T ? kPleBeT : kPleBeS) + x * he;
        return true;
    };
    for (uint32_t p = 0; p < 32; ++p) {
        uint32_t hk, r;
        mmoe_slot(p, &hk, &r);
        // the level-1 gate block
        if (hk == 0 && r < 4 * T) {
            const uint32_t t = r / 4, c = r % 4, n = Et + Es;
            if (c < 2 ? c < Et : c - 2 < Es) {
                const uint32_t col = c < 2 ? c : Et + c - 2;
                row1(o->rec.data(), PL == 2 ? 3 : 1, p, p, arr(0, kPleWgT) + (size_t)t * din * n, n, col, arr(0, kPleBgT)[t * n + col]);
            }
        }
        if (hk == 1 && r < 8 && NL == 2) {
            const uint32_t n = T * Et + Es;
            const bool ok = r < 6 ? (r / 2 < T && r % 2 < Et) : r - 6 < Es;
            const uint32_t col = r < 6 ? (r / 2) * Et + r % 2 : T * Et + r - 6;
            if (ok) row1(o->rec.data(), PL == 2 ? 3 : 1, p, p, arr(0, kPleWgS), n, col, arr(0, kPleBgS)[col]);
        }
        // the expert blocks of both levels
        for (uint32_t l = 0; l < NL; ++l)
            for (uint32_t s = 0; s < S; ++s)
                for (uint32_t gi = 0; gi <= T; ++gi) {
                    const uint32_t g = gi ? gi - 1 : T, ri = s * (T + 1) + gi, j = 16 * s + 8 * hk + (r & 7);
                    uint8_t* const rec = record(l, ri);
                    const float *W = nullptr, *b = nullptr;
                    if (!expert(l, g, r >> 3, &W, &b)) continue;
                    if (l == 0) {
                        row1(rec, P1, p, 32 + 32 * ri + p, W, he, j, b[j]);
                        continue;
                    }
                    o->be2[(size_t)ri * 32 + p] = b[j];
                    for (uint32_t ks = 0; ks < 4; ++ks)
                        for (uint32_t hh = 0; hh < 2; ++hh) {
                            float v[8];
                            for (uint32_t e = 0; e < 8; ++e) v[e] = W[(size_t)(ks * 16 + 8 * hh + e) * he + j];
                            frag_put(rec, ks, hh * 32 + p, v, PL);
                        }
                }
    }
    // the towers' slices behind the last level's task records
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t hb = 0; hb < HB; ++hb)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    float v[8];
                    for (uint32_t e = 0; e < 8; ++e) v[e] = wt[((size_t)t * he + 16 * s + 8 * (lane >> 5) + e) * ht + 32 * hb + (lane & 31)];
                    frag_put(record(NL - 1, s * (T + 1) + 1 + t), (NL == 2 ? 4 : KS) + hb, lane, v, PL);
                }
    // the second level's task gates: fp32 chains in the kernel, so plain floats in the operand precision
    if (NL == 2) {
        float* const g2 = reinterpret_cast<float*>(o->rec.data() + gfrag);
        const uint32_t n = Et + Es;
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t c = 0; c < 4; ++c) {
                if (!(c < 2 ? c < Et : c - 2 < Es)) continue;
                const uint32_t col = c < 2 ? c : Et + c - 2;
                for (uint32_t j = 0; j < 64; ++j) g2[(t * 64 + j) * 4 + c] = round_prec(arr(1, kPleWgT)[((size_t)t * he + j) * n + col], m->prec);
                o->bg2[t * 4 + c] = arr(1, kPleBgT)[t * n + col];
            }
    }
}

// PG_MODEL_DCN: where rank_dcn.hip wants each weight.  The kernel's feature order g = 0 .. dc_dp - 1 puts the item columns first,
// then the user columns, then the zero padding (dcn_source: g's index in the blob's [user | item] order).  Candidates sit on the
// MFMA column axis and a lane (item, half hk) keeps a 32-feature block of x_l, of a bias or of an accumulator as 16 registers:
// register r is feature 16 (r >> 3) + 8 hk + (r & 7) of the block — registers 0..7 and 8..15 are exactly the 8 k-values the lane
// supplies as the next product's B operand for the block's two 16-deep slices.  Since the accumulator puts row p of a block in
// (hk, r) = mmoe_slot(p), output row p of a block is made feature dcn_row(p) of it: only the OUTPUT columns of a matrix are
// permuted, its input rows and every vector stay in feature order.
inline uint32_t dcn_row(uint32_t p) {
    uint32_t hk, r;
    mmoe_slot(p, &hk, &r);
    return 16 * (r >> 3) + 8 * hk + (r & 7);
}
inline int dcn_source(uint32_t g, uint32_t du, uint32_t di) { return g < di ? (int)(du + g) : (g < du + di ? (int)(g - di) : -1); }
// a record: the two k-slices of one 32-wide input block against every 32-row output block (out / 32 fragments per slice)
constexpr size_t dcn_rec_bytes(uint32_t out, int prec) { return (size_t)2 * (out / 32) * (prec == 2 ? 2 : 1) * 1024; }
struct DcnPacked {
    std::vector<float> wu, bc;
    std::vector<uint8_t> rec;
};
// Records in the order the kernel consumes them: layer 0 (item input blocks only: the user half is c0), layers 1 .. L-1, w1, w2.
// Fragment s (out / 32) + b of a record (1 KiB; split bf16: its lo fragment follows): lane (p, hk') = input features
// 32 kb + 16 s + 8 hk' + 0..7, output feature 32 b + dcn_row(p).
inline void pack_dcn(const pg_model* m, const float* wc, const float* bc, const float* w1, const float* w2, DcnPacked* o) {
    const uint32_t du = m->d_user, di = m->d_item, D = du + di, DP = m->dc_dp, L = m->n_cross, h1 = m->h1, h2 = m->h2;
    const uint32_t PL = m->prec == 2 ? 2 : 1;
    o->wu.assign((size_t)du * DP, 0.0f);
    o->bc.assign((size_t)L * DP, 0.0f);
    for (uint32_t g = 0; g < DP; ++g) {
        const int c = dcn_source(g, du, di);
        if (c < 0) continue;
        for (uint32_t k = 0; k < du; ++k) o->wu[(size_t)k * DP + g] = round_prec(wc[(size_t)k * D + c], m->prec);
        for (uint32_t l = 0; l < L; ++l) o->bc[(size_t)l * DP + g] = bc[(size_t)l * D + c];
    }
    // W [.][ncol]: its first nkb 32-wide input blocks against `out` output features; cross_in / cross_out: that side is in the
    // kernel's feature order (dcn_source), otherwise in the blob's
    auto matrix = [&](const float* W, uint32_t ncol, uint32_t nkb, uint32_t out, bool cross_in, bool cross_out) {
        const uint32_t NBO = out / 32;
        const size_t at = o->rec.size(), rb = dcn_rec_bytes(out, m->prec);
        o->rec.resize(at + nkb * rb, 0);
        for (uint32_t kb = 0; kb < nkb; ++kb)
            for (uint32_t s = 0; s < 2; ++s)
                for (uint32_t b = 0; b < NBO; ++b)
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        const uint32_t go = 32 * b + dcn_row(lane & 31);
                        const int col = cross_out ? dcn_source(go, du, di) : (int)go;
                        uint16_t* const d = reinterpret_cast<uint16_t*>(o->rec.data() + at + kb * rb + (size_t)(s * NBO + b) * PL * 1024 + lane * 16);
                        for (uint32_t e = 0; e < 8; ++e) {
                            const uint32_t gi = 32 * kb + 16 * s + 8 * (lane >> 5) + e;
                            const int row = cross_in ? dcn_source(gi, du, di) : (int)gi;
                            float rest = row < 0 || col < 0 ? 0.0f : W[(size_t)row * ncol + col];
                            for (uint32_t pl = 0; pl < PL; ++pl) {
                                d[512 * pl + e] = f32_to_bf16_rne(rest);
                                rest -= bf16_to_f32(d[512 * pl + e]);       // (exact)
                            }
                        }
                    }
    };
    o->rec.clear();
    for (uint32_t l = 0; l < L; ++l) matrix(wc + (size_t)l * D * D, D, l ? DP / 32 : di / 32, DP, true, true);
    matrix(w1, h1, DP / 32, h1, true, false);
    matrix(w2, h2, h1 / 32, h2, false, false);
}

// PG_MODEL_MHA: where rank_mha.hip wants each weight.  Candidates sit on the MFMA column axis and a lane (candidate, half hk) holds
// rows p = (r & 3) + 8 (r >> 2) + 4 hk of a 32-row accumulator block, (hk, r) = mmoe_slot(p).  mha_row(p) is the feature of the
// block that row p is made to hold, so that register r is the feature the lane supplies as the next product's B operand: in the
// BF16 form 16 (r >> 3) + 8 hk + (r & 7) (dcn_row: registers 0..7 and 8..15 are the two 16-deep slices), in the F32 form 2 r + hk
// (register r is step r of the 2-deep MFMA).  Permuted by it, within each 32-wide block and so within each head: the OUTPUT columns
// of Wq (and bq), whose accumulators meet K in feature order in the logit product, and the output columns of Wv (and bv), whose
// P.V accumulators meet Wo's input rows in feature order.  Wk and Wo keep the blob's order.  Nothing is scaled here: the kernel
// applies log2(e) / sqrt(d_h) inside the exponent, so Wq is rounded (BF16 form) from the blob's value.
inline uint32_t mha_row(uint32_t p, bool bf16) {
    uint32_t hk, r;
    mmoe_slot(p, &hk, &r);
    return bf16 ? 16 * (r >> 3) + 8 * hk + (r & 7) : 2 * r + hk;
}
struct MhaPacked {
    std::vector<float> bq, wv, bv;
    std::vector<uint8_t> wq, wo;
};
inline void pack_mha(const pg_model* m, const float* wq, const float* bq, const float* wv, const float* bv, const float* wo, MhaPacked* o) {
    const uint32_t da = m->mh_datt;
    const bool bf16 = m->prec == 1;         // split bf16 (prec 2) runs the F32 attention in front of its trunk
    std::vector<float> wqp((size_t)kDinD * da);
    o->bq.resize(da); o->bv.resize(da); o->wv.resize((size_t)kDinD * da);
    for (uint32_t c = 0; c < da; ++c) {
        const uint32_t src = (c & ~31u) + mha_row(c & 31u, bf16);
        o->bq[c] = bq[src];
        o->bv[c] = bv[src];
        for (uint32_t k = 0; k < (uint32_t)kDinD; ++k) {
            wqp[(size_t)k * da + c] = wq[(size_t)k * da + src];
            o->wv[(size_t)k * da + c] = wv[(size_t)k * da + src];
        }
    }
    o->wq = pack_weights(wqp.data(), kDinD, da, bf16 ? 1 : 0);
    o->wo = pack_weights(wo, da, kDinD, bf16 ? 1 : 0);
}

// PG_MODEL_GBDT: the forest as rank_gbdt.hip walks it.  Tree t's record (gbdt_tree_bytes) sits at byte t * gbdt_tree_bytes of the
// buffer, so chunk c is bytes [c, c + 1) * kGbdtChunkBytes; the last chunk is zero-filled behind the last tree.  A record is the
// blob's tree with every level REVERSED: heap index m (root 1) has its left child at 2m + 1 and its right child at 2m, so the walk
// shifts the compare's outcome in.  Node slot m - 1 at 8 (m - 1) = { word, thr } — one 8-byte LDS read per visit —, slot 2^d - 1
// unused, then the leaves at 8 << d, reversed as well.  word: the feature index in bits 0..6 (the walk multiplies the low 24
// bits by the feature rows' pitch) and the missing-left flag in bits 30 AND 31: word >> 30 is then the NaN class mask.
inline std::vector<uint8_t> pack_gbdt(const pg_model* m, const uint8_t* trees, size_t blob_tree_bytes) {
    const uint32_t d = m->gb_depth, tpc = gbdt_chunk_trees(d), nn = (1u << d) - 1, nl = nn + 1;
    const size_t rec = gbdt_tree_bytes(d);
    std::vector<uint8_t> out((size_t)((m->gb_ntree + tpc - 1) / tpc) * kGbdtChunkBytes, 0);
    for (uint32_t t = 0; t < m->gb_ntree; ++t) {
        const uint8_t* const src = trees + t * blob_tree_bytes;
        uint8_t* const dst = out.data() + t * rec;
        for (uint32_t s = 0; s < d; ++s)
            for (uint32_t o = 0; o < (1u << s); ++o) {
                const uint32_t n = (1u << s) - 1 + o, slot = (2u << s) - 2 - o;      // blob node n -> heap index 2^s + (2^s - 1 - o), less 1
                uint32_t w;
                memcpy(&w, src + 4 * n, 4);
                w = (w & 0x7Fu) | ((w >> 31) * 0xC0000000u);
                memcpy(dst + 8 * slot, &w, 4);
                memcpy(dst + 8 * slot + 4, src + 4 * (nn + n), 4);
            }
        for (uint32_t l = 0; l < nl; ++l) memcpy(dst + 8 * (size_t)nl + 4 * (nl - 1 - l), src + 4 * (size_t)(2 * nn + l), 4);
    }
    return out;
}

// ---- what goes to the device ---------------------------------------------------------------------------------------------
// One allocation of a loaded model: `bytes` from `src` (the blob, or a buffer ModelUploads owns) into a device buffer whose
// address *dst receives; `lo`: the member that points at the second half of that buffer (the lo fragments of split operands).
struct ModelUpload {
    void** dst;
    const void* src;
    size_t bytes;
    void** lo;
};
inline void model_upload_placed(const ModelUpload& u, void* d) {
    *u.dst = d;
    if (u.lo) *u.lo = (char*)d + u.bytes / 2;
}
struct ModelUploads {
    std::vector<ModelUpload> list;                 // in allocation order
    std::vector<std::vector<float>> floats;        // what the entries point into beside the blob
    std::vector<std::vector<uint8_t>> packed;
};

// The uploads of a parsed blob (*m and lay from parse_model_blob), every entry's destination a member of *m.  The two-tower
// model's field-pointer arrays are not among them: they hold device addresses inside `fields`, so the loader builds them last.
inline int model_uploads(pg_model* m, const BlobLayout& lay, const void* blob, ModelUploads* up, ModelRefusal* why) {
    const uint8_t* p = (const uint8_t*)blob;
    auto at = [&](size_t off) { return (const float*)(p + off); };
    auto add = [&](auto* dst, const void* src, size_t bytes, void** lo = nullptr) { up->list.push_back({(void**)dst, src, bytes, lo}); };
    auto add_floats = [&](auto* dst, std::vector<float>&& v) {
        up->floats.push_back(std::move(v));
        add(dst, up->floats.back().data(), up->floats.back().size() * 4);
    };
    auto add_packed = [&](void** dst, std::vector<uint8_t>&& v, void** lo) {
        up->packed.push_back(std::move(v));
        add(dst, up->packed.back().data(), up->packed.back().size(), lo);
    };
    if (m->kind == PG_MODEL_DCN) {
        DcnPacked pk;
        pack_dcn(m, at(lay.wc), at(lay.bc), at(lay.w1), at(lay.w2), &pk);
        const float* w3 = at(lay.w3);
        std::vector<float> w3t((size_t)m->n_out * m->h2);          // head-major, as a DNN3's
        for (uint32_t o = 0; o < m->n_out; ++o)
            for (uint32_t j = 0; j < m->h2; ++j) w3t[(size_t)o * m->h2 + j] = w3[(size_t)j * m->n_out + o];
        add_floats(&m->dc_wu, std::move(pk.wu));
        add_floats(&m->dc_bc, std::move(pk.bc));
        add_packed(&m->dc_rec, std::move(pk.rec), nullptr);
        add(&m->b1, at(lay.b1), (size_t)m->h1 * 4);
        add(&m->b2, at(lay.b2), (size_t)m->h2 * 4);
        add_floats(&m->w3, std::move(w3t));
        add(&m->b3v, at(lay.b3), (size_t)m->n_out * 4);
    } else if (m->kind == PG_MODEL_GBDT) {
        add_packed(&m->gb_forest, pack_gbdt(m, p + lay.gb_trees, lay.gb_tree_bytes), nullptr);
    } else if (m->kind == PG_MODEL_MIND) {         // [in][out] is the order the kernel reads: the arrays go up as they are
        add(&m->mi_w, p + 24, MindLayout(m->d_user, m->mi_dout, m->n_out, m->h1).floats * 4);
    } else if (m->kind == PG_MODEL_MMOE) {
        MmoePacked pk;
        pack_mmoe(m, at(lay.we), at(lay.be), at(lay.wg), at(lay.bg), at(lay.wt), at(lay.bt), at(lay.wo), at(lay.bo), &pk);
        add_floats(&m->mm_wu, std::move(pk.wu));
        add_floats(&m->mm_bu, std::move(pk.bu));
        add_packed(&m->mm_rec, std::move(pk.rec), nullptr);
        add_floats(&m->mm_bt, std::move(pk.bt));
        add_floats(&m->mm_wo, std::move(pk.wo));
        add_floats(&m->mm_bo, std::move(pk.bo));
    } else if (m->kind == PG_MODEL_PLE) {
        PlePacked pk;
        pack_ple(m, p, lay, &pk);
        add_floats(&m->mm_wu, std::move(pk.wu));
        add_floats(&m->mm_bu, std::move(pk.bu));
        add_packed(&m->mm_rec, std::move(pk.rec), nullptr);
        add_floats(&m->pl_be2, std::move(pk.be2));
        add_floats(&m->pl_bg2, std::move(pk.bg2));
        add_floats(&m->mm_bt, std::move(pk.bt));
        add_floats(&m->mm_wo, std::move(pk.wo));
        add_floats(&m->mm_bo, std::move(pk.bo));
    } else if (m->kind == PG_MODEL_DNN3 || m->kind == PG_MODEL_DIN || m->kind == PG_MODEL_MHA) {
        const float *w1 = at(lay.w1), *w2 = at(lay.w2), *w3 = at(lay.w3);
        // a DIN's or an MHA's trunk is a DNN3 over the staged rows [e | pooled]: the item half of w1 is those 128 rows
        const uint32_t item_rows = m->kind == PG_MODEL_DNN3 ? m->d_item : 2 * m->d_item;
        if (m->kind == PG_MODEL_MHA) {
            MhaPacked pk;
            pack_mha(m, at(lay.a_wq), at(lay.a_bq), at(lay.a_wv), at(lay.a_bv), at(lay.a_wo), &pk);
            add_packed(&m->mh_wq, std::move(pk.wq), nullptr);
            add_floats(&m->mh_bq, std::move(pk.bq));
            add(&m->mh_wk, at(lay.a_wk), (size_t)kDinD * m->mh_datt * 4);
            add_floats(&m->mh_wv, std::move(pk.wv));
            add_floats(&m->mh_bv, std::move(pk.bv));
            add_packed(&m->mh_wo, std::move(pk.wo), nullptr);
        }
        if (m->kind == PG_MODEL_DIN) {
            std::vector<float> wq, wk, wp;
            fold_din_attention(at(lay.wa), m->att_h, &wq, &wk, &wp);
            add_floats(&m->att_wq, std::move(wq));
            add_floats(&m->att_wk, std::move(wk));
            add_floats(&m->att_wp, std::move(wp));
            add(&m->att_ba, at(lay.ba), (size_t)m->att_h * 4);
            add(&m->att_wa2, at(lay.wa2), (size_t)m->att_h * 4);
        }
        std::vector<float> w3t((size_t)m->n_out * m->h2);          // kept head-major on the device
        for (uint32_t o = 0; o < m->n_out; ++o)
            for (uint32_t j = 0; j < m->h2; ++j) w3t[(size_t)o * m->h2 + j] = w3[(size_t)j * m->n_out + o];
        // the kernel's layer 1 is 128 deep: a 64-wide item row is padded with zero columns, W1 with zero rows
        std::vector<float> w1i((size_t)kDIN * m->h1, 0.0f);
        memcpy(w1i.data(), w1 + (size_t)m->d_user * m->h1, (size_t)item_rows * m->h1 * 4);
        void** const split = m->prec == 2 ? &m->w1p_lo : nullptr;   // split bf16: the lo fragments follow the hi fragments
        add_floats(&m->w1u, rounded(w1, (size_t)m->d_user * m->h1, m->prec));
        add(&m->b1, at(lay.b1), (size_t)m->h1 * 4);
        add_packed(&m->w1p, pack_weights(w1i.data(), kDIN, m->h1, m->prec), split);
        add_packed(&m->w2p, pack_weights(w2, m->h1, m->h2, m->prec), split ? &m->w2p_lo : nullptr);
        add(&m->b2, at(lay.b2), (size_t)m->h2 * 4);
        add_floats(&m->w3, std::move(w3t));
        add(&m->b3v, at(lay.b3), (size_t)m->n_out * 4);
        if (m->f16_nprod) {
            std::vector<uint8_t> hw1, hw2;
            std::vector<float> xs, hs;
            int rc;
            if ((rc = build_f16_operands(w1i.data(), w2, m->h1, m->h2, m->f16_nprod, &hw1, &hw2, &xs, &hs, why))) return rc;
            const bool two = m->f16_nprod == 2;
            add_packed(&m->h_w1p, std::move(hw1), two ? &m->h_w1p_lo : nullptr);
            add_packed(&m->h_w2p, std::move(hw2), two ? &m->h_w2p_lo : nullptr);
            add_floats(&m->h_xs, std::move(xs));
            add_floats(&m->h_hs, std::move(hs));
            add_floats(&m->h_stats, std::vector<float>(4, 0.0f));      // two 64-bit counters, zero
        }
    } else {
        const uint32_t din = m->nif * m->k;
        void** const split = m->prec == 2 ? &m->w1p_lo : nullptr;
        add_floats(&m->w1u, rounded(at(lay.uw1), (size_t)m->d_user * m->th, m->prec));
        add(&m->b1, at(lay.ub1), (size_t)m->th * 4);
        add_floats(&m->uw2, rounded(at(lay.uw2), (size_t)m->th * m->to, m->prec));
        add(&m->ub2, at(lay.ub2), (size_t)m->to * 4);
        add_packed(&m->w1p, pack_weights(at(lay.iw1), din, m->th, m->prec), split);
        add(&m->c1_shared, at(lay.ib1), (size_t)m->th * 4);
        add_packed(&m->w2p, pack_weights(at(lay.iw2), m->th, m->to, m->prec), split ? &m->w2p_lo : nullptr);
        add(&m->b2, at(lay.ib2), (size_t)m->to * 4);
        add(&m->fields, at(lay.fields), lay.field_floats * 4);
    }
    return PG_OK;
}

}  // namespace pg
