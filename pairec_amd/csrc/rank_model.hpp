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
};

// What `blob` says as a model of `kind` in `prec`: the dimensions (and kind, prec, f16_nprod, b3, fm_b) into *m, the arrays'
// offsets into *lay.  PG_OK, or the refusal in *why.
inline int parse_model_blob(int kind, int prec, const void* blob, size_t len, pg_model* m, BlobLayout* lay, ModelRefusal* why) {
    if (!(prec == PG_PREC_F32 || prec == PG_PREC_BF16 || prec == PG_PREC_BF16X3 || prec == PG_PREC_F16X2 || prec == PG_PREC_F16))
        return refuse(why, PG_ERR_INVALID, "pg_model_load: bad precision %d", prec);
    const int f16_nprod = prec == PG_PREC_F16X2 ? 2 : (prec == PG_PREC_F16 ? 1 : 0);
    if (f16_nprod && kind == PG_MODEL_FM_TWOTOWER)
        return refuse(why, PG_ERR_UNSUPPORTED, "pg_model_load: PG_PREC_F16X2 / PG_PREC_F16 serve PG_MODEL_DNN3 and PG_MODEL_DNN3_MULTI; load a "
                                               "PG_MODEL_FM_TWOTOWER in PG_PREC_BF16X3");
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
    if (m->kind == PG_MODEL_DNN3) {
        const float *w1 = at(lay.w1), *w2 = at(lay.w2), *w3 = at(lay.w3);
        std::vector<float> w3t((size_t)m->n_out * m->h2);          // kept head-major on the device
        for (uint32_t o = 0; o < m->n_out; ++o)
            for (uint32_t j = 0; j < m->h2; ++j) w3t[(size_t)o * m->h2 + j] = w3[(size_t)j * m->n_out + o];
        // the kernel's layer 1 is 128 deep: a 64-wide item row is padded with zero columns, W1 with zero rows
        std::vector<float> w1i((size_t)kDIN * m->h1, 0.0f);
        memcpy(w1i.data(), w1 + (size_t)m->d_user * m->h1, (size_t)m->d_item * m->h1 * 4);
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
