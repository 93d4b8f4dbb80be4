// rank_mha.hip — PG_MODEL_MHA: multi-head scaled dot-product softmax attention of every candidate over the request's behaviour
// sequence (up to PG_MHA_MAX_SEQ = 512 rows), in front of the DNN3 trunk.
//
// The reference carries a user's sequence as a first-class feature (Feature_Type_Sequence, module/feature_dao.go:19, 94-134;
// SequenceLength, recconf/recconf.go:202-212) with no bound of 64 on it, and ships it to remote EasyRec models whose sequence
// blocks (BST, multi-head target attention) are softmax attention.  Here, e a candidate row, s_l the
// request's VALID sequence rows (the first min(len, 512) entries that name a row of the table):
//     q = Wq' e + bq      K_l = Wk' s_l      V_l = Wv' s_l + bv                                        (d_att wide, H heads of d_h)
//     per head h:  a_l = q_h . K_lh / sqrt(d_h)     p = softmax_l(a)     o_h = sum_l p_l V_lh
//     pooled = Wo' [o_0 | .. | o_{H-1}]     (64)    staged as [e | pooled] for the unchanged trunk, as rank_din.hip does
//
// Two kernels.  A request's K and V are shared by all its candidates (about 40 tiles of 128 at 5 000 candidates), so they are
// projected ONCE per request by mha_kv_kernel and only streamed by mha_attn_kernel.
//
// mha_kv_kernel, one workgroup per request of the run.  It drops the invalid entries by ballot rank (an entry past the table is
// LEFT OUT of the softmax: a zero key would still take weight), writes n_valid[r], gathers the valid rows 32 positions at a
// time, projects K and V as fp32 fmaf chains over d ascending (thread = one column of [K | V]; nothing is rounded inside the
// projection) and writes the block to scratch as one RECORD in MFMA fragment order — bf16 (RNE, once) for the BF16 form, fp32 for
// the F32 form; the tail of the last block is zero-filled.
//
// mha_attn_kernel, one workgroup of 4 waves per tile of up to 128 candidates of one request (the trunk's tile builder), candidates
// on the MFMA COLUMN axis: wave w the candidates 32 w .. 32 w + 31, lane (j, hk) candidate j.  In a 32 x 32 accumulator block a
// lane owns rows p = (r & 3) + 8 (r >> 2) + 4 hk, r = 0..15, of its candidate's column.
//   q.        A lane reads its candidate's row straight into operand registers (and writes the fp32 values to the staging row);
//             q^T = Wq^T . e on accumulators that start at bq.  rank_model.hpp (pack_mha, mha_row) permutes Wq's output columns
//             within each 32-wide block so that accumulator register r holds exactly the feature the lane must supply as the B
//             operand of the logit product: BF16  16 (r >> 3) + 8 hk + (r & 7)  (registers 0..7 / 8..15 = the two 16-deep
//             slices), F32  2 r + hk  (register r = step r of the 2-deep MFMA).  The q accumulators ARE the operand registers
//             (converted once in BF16); K is stored in the matching feature order — a dot product does not care about a common
//             permutation of its terms.
//   logits.   S[32 pos x 32 cand] = K_blk[32 x d_h] . q_h[d_h x 32]: a lane holds 16 positions of one candidate, its partner
//             lane (j, 1 - hk) the other 16.
//   softmax.  Online, in registers: block max = in-lane reduction + ONE exchange between the lane halves; the head's O
//             accumulators and l are rescaled only when some lane's max moved (a ballot); l sums the UNROUNDED p per lane half
//             and the halves are combined once at the end.  The scale log2(e) / sqrt(d_h) is applied inside the exponent's fma,
//             p = v_exp_f32(fma(s, c, -m c)): the same instruction count as a folded Wq, and the BF16 form's rounding points
//             stay exactly those of the specification (Wq and q are rounded, not Wq c and q c).
//   P.V.      The order of positions inside a block is free (softmax and the weighted sum are permutation-invariant), so the
//             prologue writes V's fragments in the position order in which the logit accumulators ALREADY sit in each lane:
//             O^T[d_h x 32 cand] += V_blk^T[d_h x 32 pos] . P with P's B operand = the p registers, converted (BF16) or as they
//             are (F32).  No LDS round trip, no cross-lane shuffle.
//   tail.     Positions >= n_valid of the last block get a logit of -inf by index (their K and V are zero).  n_valid = 0 skips
//             the loop: the first block always holds a valid position, so m is finite from then on; pooled is then 0.
//   Wo.       pooled^T = Wo^T . (o / l) runs on the O accumulators as B operands (the loader permutes V's output columns by the
//             same mha_row, Wo's input rows stay in feature order); [e | pooled] goes to the staging row.
//
// LDS holds one stream of equal-sized records, double-buffered as rank_dcn.hip's: Wq, the request's K/V blocks, Wo.  A record
// is 64 x d_att operand values of Wq = K (32 x d_att) + V (32 x d_att) of a block = d_att x 64 of Wo:
//     BF16: 8 KB (d_att 64) / 16 KB (128) per buffer, 16 / 32 KB per workgroup — two workgroups (and more) per CU of the 160 KB
//     F32:  16 KB / 32 KB per buffer, 32 / 64 KB per workgroup
//     [0, RB) buffer 0 | [RB, 2 RB) buffer 1;  record i lives in buffer i & 1, fragment f of it at f KiB, lane's 16 B at 16 lane
//     BF16 K/V record: K fragment ks (d_att / 16): lane (pos i, hk) = K[i][16 ks + 8 hk + 0..7];
//                      V fragment 2 ob + s: lane (row i, hk) = V'[pos (e & 3) + 8 (e >> 2) + 4 hk + 16 s][32 ob + i], e = 0..7
//     F32  K/V record: K fragment 4 b + g (d_att / 8): lane (pos i, hk) = K[i][32 b + 8 g + 2 x + hk], x = 0..3;
//                      V fragment 4 ob + g: lane (row i, hk) = V'[pos x + 8 g + 4 hk][32 ob + i]
//
// Two forms.  F32 (PG_PREC_F32, and in front of the split-bf16 trunk of PG_PREC_BF16X3): v_mfma_f32_32x32x2_f32, nothing in
// the attention is rounded.  BF16: v_mfma_f32_32x32x16_bf16; rounded once, RNE: e as Wq's operand and Wq; q as the logit
// product's operand; K and V as stored; the unnormalised p = exp(a - m) as the P.V operand; the normalised o as Wo's operand and
// Wo.  Kept fp32: the K/V projection itself, every accumulation, the running max m, the exponent, the running sum l (of the
// unrounded p), the rescale and 1 / l, pooled as staged.
//
// Runs.  As rank_din.hip: kDinRunItems staged candidates per run, and at most kMhaRunReqs requests, which bounds a run's K/V
// scratch at 256 x 512 x d_att x 2 x 4 B = 128 MB whatever the call's size.
#include "rank_mlp.hpp"

#include <algorithm>

namespace pg {

constexpr int kMhaBlock = 32;                                   // positions per K/V record
constexpr int kMhaMaxBlocks = PG_MHA_MAX_SEQ / kMhaBlock;       // records per request

constexpr int mha_rec_bytes(int bf16, int datt) { return kDinD * datt * (bf16 ? 2 : 4); }

struct MhaKvArgs {
    const uint32_t* loc_off;        // the run's offsets: a request with no candidate in the run is skipped
    const float* tab;
    uint32_t tab_rows;
    const uint32_t* seq_rows;
    const uint32_t* seq_off;        // the run's first request
    const float *wk, *wv, *bv;      // [64][d_att] fp32 (wv, bv: columns in mha_row order)
    uint32_t* n_valid;              // [run requests]
    char* kv;                       // [run requests][kMhaMaxBlocks] records
};

struct MhaArgs {
    const uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles;
    const float* tab;
    uint32_t tab_rows;
    const uint32_t* cand_rows;      // the run's first candidate
    const uint32_t* n_valid;
    const char* kv;
    const char *wq, *wo;            // one record each
    const float* bq;                // [d_att], in accumulator-row order
    float* stage;                   // [run items][kDIN]
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t mha_cvt2(float a, float b) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));      // v_cvt_pk_bf16_f32 (RNE)
}
// registers 8 s .. 8 s + 7 of an accumulator block as a bf16 B operand
__device__ __forceinline__ bf16x8 mha_operand(const f32x16& v, int s) {
    const u32x4_t p = {mha_cvt2(v[8 * s], v[8 * s + 1]), mha_cvt2(v[8 * s + 2], v[8 * s + 3]), mha_cvt2(v[8 * s + 4], v[8 * s + 5]),
                       mha_cvt2(v[8 * s + 6], v[8 * s + 7])};
    return __builtin_bit_cast(bf16x8, p);
}

// ---- the K/V prologue ----------------------------------------------------------------------------------------------------------
template <int BF16, int DATT>
__global__ __launch_bounds__(256) void mha_kv_kernel(MhaKvArgs a) {
    constexpr int D = kDinD;
    constexpr int NC = 2 * DATT;                  // columns of [K | V]
    constexpr int NCP = NC + 1;                   // ... padded: a fragment's 32 rows of one column fall in 32 banks
    constexpr int NG = 256 / NC;                  // positions computed side by side (1 or 2)
    constexpr int RB = mha_rec_bytes(BF16, DATT);
    constexpr int NU = RB / 16 / 256;             // 16-B fragment entries per thread and record
    __shared__ uint32_t rows[PG_MHA_MAX_SEQ];
    __shared__ uint32_t wcnt[4];
    __shared__ __attribute__((aligned(16))) float S[kMhaBlock * D];
    __shared__ __attribute__((aligned(16))) float KV[kMhaBlock * NCP];

    const uint32_t r = blockIdx.x;
    if (a.loc_off[r + 1] == a.loc_off[r]) return;                     // no candidate of the run reads this request
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t s0 = a.seq_off[r], s1 = a.seq_off[r + 1];
    const int L = s1 > s0 ? (s1 - s0 < (uint32_t)PG_MHA_MAX_SEQ ? (int)(s1 - s0) : PG_MHA_MAX_SEQ) : 0;

    // ---- the valid entries, in order: rank by ballot within a wave, by the waves' counts across them ---------------------------
    int nv = 0;
    for (int base = 0; base < L; base += 256) {
        const int pos = base + tid;
        uint32_t row = 0;
        bool ok = false;
        if (pos < L) {
            row = a.seq_rows[s0 + pos];
            ok = row < a.tab_rows;
        }
        const unsigned long long b = __ballot(ok);
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        int before = nv;
        for (int w = 0; w < wave; ++w) before += (int)wcnt[w];
        if (ok) rows[before + __popcll(b & ((1ull << lane) - 1))] = row;
        nv += (int)(wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
        __syncthreads();
    }
    if (tid == 0) a.n_valid[r] = (uint32_t)nv;

    // ---- this thread's column of [Wk | Wv], kept across all positions -----------------------------------------------------------
    const int c = tid % NC, lg = tid / NC;
    const bool is_v = c >= DATT;
    float w[D];
#pragma unroll
    for (int d = 0; d < D; ++d) w[d] = is_v ? a.wv[d * DATT + c - DATT] : a.wk[d * DATT + c];
    const float bias = is_v ? a.bv[c - DATT] : 0.f;

    const int nb = (nv + kMhaBlock - 1) / kMhaBlock;
    for (int kb = 0; kb < nb; ++kb) {
        // the block's rows into LDS (16 lanes x 16 B per row); positions past n_valid are zero rows
        for (int i = tid; i < kMhaBlock * 16; i += 256) {
            const int l = i >> 4, pos = kb * kMhaBlock + l;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos < nv) v = *reinterpret_cast<const float4*>(a.tab + (size_t)rows[pos] * D + 4 * (i & 15));
            *reinterpret_cast<float4*>(S + l * D + 4 * (i & 15)) = v;
        }
        __syncthreads();                                              // S complete; the block before has been written out
        // KV[l][c] = bias + sum_d w[d] s_l[d], d ascending; the tail of the last block is zero, bias included
        for (int l = lg; l < kMhaBlock; l += NG) {
            float acc = bias;
#pragma unroll
            for (int d4 = 0; d4 < D / 4; ++d4) {
                const float4 sv = *reinterpret_cast<const float4*>(S + l * D + 4 * d4);
                acc = __fmaf_rn(w[4 * d4 + 0], sv.x, acc);
                acc = __fmaf_rn(w[4 * d4 + 1], sv.y, acc);
                acc = __fmaf_rn(w[4 * d4 + 2], sv.z, acc);
                acc = __fmaf_rn(w[4 * d4 + 3], sv.w, acc);
            }
            KV[l * NCP + c] = kb * kMhaBlock + l < nv ? acc : 0.f;
        }
        __syncthreads();
        // the record, 16 B per (fragment, lane)
        u32x4_t* const rec = reinterpret_cast<u32x4_t*>(a.kv + ((size_t)r * kMhaMaxBlocks + kb) * RB);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e16 = tid + 256 * u, f = e16 >> 6, ln = e16 & 63, i = ln & 31, hk = ln >> 5;
            float v[8];
            if constexpr (BF16) {
                if (f < DATT / 16) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = KV[i * NCP + 16 * f + 8 * hk + e];
                } else {
                    const int fv = f - DATT / 16, ob = fv >> 1, s = fv & 1;
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = KV[((e & 3) + 8 * (e >> 2) + 4 * hk + 16 * s) * NCP + DATT + 32 * ob + i];
                }
                rec[e16] = (u32x4_t){mha_cvt2(v[0], v[1]), mha_cvt2(v[2], v[3]), mha_cvt2(v[4], v[5]), mha_cvt2(v[6], v[7])};
            } else {
                if (f < DATT / 8) {
                    const int b = f >> 2, g = f & 3;
#pragma unroll
                    for (int x = 0; x < 4; ++x) v[x] = KV[i * NCP + 32 * b + 8 * g + 2 * x + hk];
                } else {
                    const int fv = f - DATT / 8, ob = fv >> 2, g = fv & 3;
#pragma unroll
                    for (int x = 0; x < 4; ++x) v[x] = KV[(x + 8 * g + 4 * hk) * NCP + DATT + 32 * ob + i];
                }
                rec[e16] = (u32x4_t){__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
            }
        }
    }
}

// ---- the attention ------------------------------------------------------------------------------------------------------------
template <int BF16, int DATT, int DH>
__global__ __launch_bounds__(256) void mha_attn_kernel(MhaArgs a) {
    constexpr int D = kDinD;
    constexpr int NQB = DATT / 32;                // 32-feature blocks of q and of O
    constexpr int BPH = DH / 32;                  // ... per head
    constexpr int NH = DATT / DH;
    constexpr int KF = BF16 ? D / 16 : D / 8;     // Wq: fragments per q block (k-groups of the 64-deep product)
    constexpr int OF = BF16 ? DATT / 16 : DATT / 8;   // Wo: fragments per pooled block; K/V record: K fragments (V's follow)
    constexpr int RB = mha_rec_bytes(BF16, DATT);
    constexpr int NLD = RB / 16 / 256;            // 16-B loads per thread and record
    static_assert((DATT == 64 || DATT == 128) && (DH == 32 || DH == 64) && NH >= 1 && NH <= 4, "attention shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const uint32_t tile = blockIdx.x;
    if (tile >= *a.n_tiles) return;
    const uint32_t req = a.tile_req[tile];
    const uint32_t item0 = a.tile_item0[tile];
    const uint32_t cnt = a.tile_cnt[tile];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hk = lane >> 5;
    const bool active = (uint32_t)wave * 32 < cnt;      // (wave-uniform; every wave copies records and takes the barriers)

    // ---- the record stream (rank_dcn.hip's): record i lives in buffer i & 1; a step requests the next record before its MFMAs
    // (fetch) and writes it to the other buffer, last read one step earlier, after them (commit: one barrier) ---------------------
    u32x4_t pre[NLD];
    uint32_t nrec = 0;
    auto fetch = [&](const char* src) {
#pragma unroll
        for (int c = 0; c < NLD; ++c) pre[c] = reinterpret_cast<const u32x4_t*>(src)[tid + 256 * c];
    };
    auto commit = [&]() {
        u32x4_t* const dst = reinterpret_cast<u32x4_t*>(smem + (nrec & 1) * RB);
#pragma unroll
        for (int c = 0; c < NLD; ++c) dst[tid + 256 * c] = pre[c];
        ++nrec;
        __syncthreads();
    };
    fetch(a.wq);

    // ---- this lane's candidate: its row as MFMA operand registers, the fp32 values on to the staging row ------------------------
    const uint32_t r_item = wave * 32 + j;
    const bool live = r_item < cnt;
    float* const out_row = a.stage + (size_t)(item0 + (live ? r_item : 0)) * kDIN;
    uint32_t erow = a.cand_rows[item0 + (live ? r_item : cnt - 1)];
    erow = erow < a.tab_rows ? erow : a.tab_rows - 1;
    const float4* const ep = reinterpret_cast<const float4*>(a.tab + (size_t)erow * D);
    bf16x8 eb[BF16 ? D / 16 : 1];       // BF16: lane (j, hk) holds e[16 ks + 8 hk + 0..7]
    float ef[BF16 ? 1 : D / 2];         // F32:  lane (j, hk) holds e[2 m + hk]
    if constexpr (BF16) {
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) {
            const float4 v0 = ep[ks * 4 + 2 * hk], v1 = ep[ks * 4 + 2 * hk + 1];
            if (live) {
                *reinterpret_cast<float4*>(out_row + ks * 16 + 8 * hk) = v0;
                *reinterpret_cast<float4*>(out_row + ks * 16 + 8 * hk + 4) = v1;
            }
            const u32x4_t p = {mha_cvt2(v0.x, v0.y), mha_cvt2(v0.z, v0.w), mha_cvt2(v1.x, v1.y), mha_cvt2(v1.z, v1.w)};
            eb[ks] = __builtin_bit_cast(bf16x8, p);
        }
    } else {
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            const float4 v = ep[c];
            if (live && (c >> 3) == hk) *reinterpret_cast<float4*>(out_row + 4 * c) = v;
            ef[2 * c] = hk ? v.y : v.x;
            ef[2 * c + 1] = hk ? v.w : v.z;
        }
    }
    const int nv = (int)a.n_valid[req];
    const int nb = (nv + kMhaBlock - 1) / kMhaBlock;
    const char* const kv = a.kv + (size_t)req * kMhaMaxBlocks * RB;
    commit();                                                         // Wq in buffer 0

    // ---- q^T = Wq^T . e from bq: the accumulators are the logit product's B operand ---------------------------------------------
    f32x16 q[NQB];
    {
        const char* const cur = smem + ((nrec - 1) & 1) * RB;
        fetch(nb ? kv : a.wo);
        if (active) {
#pragma unroll
            for (int b = 0; b < NQB; ++b) {
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const float4 c = *reinterpret_cast<const float4*>(a.bq + 32 * b + 8 * qd + 4 * hk);
                    q[b][4 * qd + 0] = c.x; q[b][4 * qd + 1] = c.y; q[b][4 * qd + 2] = c.z; q[b][4 * qd + 3] = c.w;
                }
                if constexpr (BF16) {
#pragma unroll
                    for (int ks = 0; ks < KF; ++ks)
                        q[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(cur + (b * KF + ks) * 1024 + lane * 16),
                                                                       eb[ks], q[b], 0, 0, 0);
                } else {
#pragma unroll
                    for (int g8 = 0; g8 < KF; ++g8) {
                        const f32x4 wf = *reinterpret_cast<const f32x4*>(cur + (b * KF + g8) * 1024 + lane * 16);
#pragma unroll
                        for (int st = 0; st < 4; ++st) q[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[st], ef[g8 * 4 + st], q[b], 0, 0, 0);
                    }
                }
            }
        }
        commit();
    }
    bf16x8 qb[BF16 ? NQB : 1][2];       // BF16: q rounded once, the two 16-deep slices of each block
    if constexpr (BF16) {
#pragma unroll
        for (int b = 0; b < NQB; ++b) {
            qb[b][0] = mha_operand(q[b], 0);
            qb[b][1] = mha_operand(q[b], 1);
        }
    }

    // ---- the sequence, a record of 32 positions at a time: logits, online softmax, P.V ------------------------------------------
    const float cs = (DH == 64 ? 0.125f : 0.17677669529663687f) * 1.4426950408889634f;      // log2(e) / sqrt(d_h)
    f32x16 O[NQB];
    float m[NH], mc[NH], lsum[NH];      // running max of the raw logits, the same scaled by cs, this lane half's sum of p
#pragma unroll
    for (int b = 0; b < NQB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[b][r] = 0.f;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        m[h] = -INFINITY;
        mc[h] = -INFINITY;
        lsum[h] = 0.f;
    }
    for (int kb = 0; kb < nb; ++kb) {
        const char* const cur = smem + ((nrec - 1) & 1) * RB;
        fetch(kb + 1 < nb ? kv + (size_t)(kb + 1) * RB : a.wo);
        if (active) {
            const int left = nv - kb * kMhaBlock;                     // valid positions from this block on
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                f32x16 s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
                for (int bb = 0; bb < BPH; ++bb) {
                    const int b = h * BPH + bb;
                    if constexpr (BF16) {
#pragma unroll
                        for (int sl = 0; sl < 2; ++sl)
                            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(cur + (2 * b + sl) * 1024 + lane * 16),
                                                                        qb[BF16 ? b : 0][sl], s, 0, 0, 0);
                    } else {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 kf = *reinterpret_cast<const f32x4*>(cur + (4 * b + g) * 1024 + lane * 16);
#pragma unroll
                            for (int x = 0; x < 4; ++x) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[x], q[b][4 * g + x], s, 0, 0, 0);
                        }
                    }
                }
                if (left < kMhaBlock) {                               // (uniform) the last block's tail: out of the softmax, by index
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if ((r & 3) + 8 * (r >> 2) + 4 * hk >= left) s[r] = -INFINITY;
                }
                float bm = s[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) bm = fmaxf(bm, s[r]);
                bm = fmaxf(bm, __shfl_xor(bm, 32));
                const float mn = fmaxf(m[h], bm), mnc = mn * cs;
                if (__ballot(mn > m[h])) {                            // some candidate's max moved: rescale (a factor of exactly 1 elsewhere)
                    const float sc = __builtin_amdgcn_exp2f(mc[h] - mnc);
                    lsum[h] *= sc;
#pragma unroll
                    for (int bb = 0; bb < BPH; ++bb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) O[h * BPH + bb][r] *= sc;
                    m[h] = mn;
                    mc[h] = mnc;
                }
                f32x16 p;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    p[r] = __builtin_amdgcn_exp2f(__fmaf_rn(s[r], cs, -mc[h]));
                    lsum[h] += p[r];
                }
                if constexpr (BF16) {
                    const bf16x8 p0 = mha_operand(p, 0), p1 = mha_operand(p, 1);
#pragma unroll
                    for (int bb = 0; bb < BPH; ++bb) {
                        const int b = h * BPH + bb;
                        O[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(cur + (OF + 2 * b) * 1024 + lane * 16), p0, O[b], 0, 0, 0);
                        O[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(cur + (OF + 2 * b + 1) * 1024 + lane * 16), p1, O[b], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int bb = 0; bb < BPH; ++bb) {
                        const int b = h * BPH + bb;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 vf = *reinterpret_cast<const f32x4*>(cur + (OF + 4 * b + g) * 1024 + lane * 16);
#pragma unroll
                            for (int x = 0; x < 4; ++x) O[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[x], p[4 * g + x], O[b], 0, 0, 0);
                        }
                    }
                }
            }
        }
        commit();
    }
    if (!active) return;

    // ---- pooled^T = Wo^T . (o / l) on the O accumulators; Wo is the record now in LDS -------------------------------------------
    const char* const cur = smem + ((nrec - 1) & 1) * RB;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const float lt = lsum[h] + __shfl_xor(lsum[h], 32);
        const float inv = nv ? 1.0f / lt : 0.f;
#pragma unroll
        for (int bb = 0; bb < BPH; ++bb)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[h * BPH + bb][r] *= inv;
    }
    f32x16 pl[2];
#pragma unroll
    for (int nbg = 0; nbg < 2; ++nbg) {
#pragma unroll
        for (int r = 0; r < 16; ++r) pl[nbg][r] = 0.f;
#pragma unroll
        for (int b = 0; b < NQB; ++b) {
            if constexpr (BF16) {
#pragma unroll
                for (int sl = 0; sl < 2; ++sl)
                    pl[nbg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(cur + (nbg * OF + 2 * b + sl) * 1024 + lane * 16),
                                                                      mha_operand(O[b], sl), pl[nbg], 0, 0, 0);
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 wf = *reinterpret_cast<const f32x4*>(cur + (nbg * OF + 4 * b + g) * 1024 + lane * 16);
#pragma unroll
                    for (int x = 0; x < 4; ++x) pl[nbg] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[x], O[b][4 * g + x], pl[nbg], 0, 0, 0);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int nbg = 0; nbg < 2; ++nbg)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
                *reinterpret_cast<float4*>(out_row + D + 32 * nbg + 8 * qd + 4 * hk) =
                    make_float4(pl[nbg][4 * qd], pl[nbg][4 * qd + 1], pl[nbg][4 * qd + 2], pl[nbg][4 * qd + 3]);
    }
}

template <int BF16, int DATT, int DH>
static int launch_mha(pg_ctx* ctx, const MhaKvArgs& ka, uint32_t n_req, const MhaArgs& a, uint32_t grid) {
    constexpr size_t lds = 2 * (size_t)mha_rec_bytes(BF16, DATT);
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)mha_attn_kernel<BF16, DATT, DH>, lds))) return rc;
    mha_kv_kernel<BF16, DATT><<<n_req, 256, 0, ctx->stream>>>(ka);
    PG_HIP(hipGetLastError());
    mha_attn_kernel<BF16, DATT, DH><<<grid, 256, lds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
template <int BF16>
static int launch_mha_shape(pg_ctx* ctx, const pg_model* m, const MhaKvArgs& ka, uint32_t n_req, const MhaArgs& a, uint32_t grid) {
#define X(A, H)                                           \
    if (m->mh_datt == A && m->mh_heads == H) return launch_mha<BF16, A, A / H>(ctx, ka, n_req, a, grid);
    PG_MHA_SHAPES(X)
#undef X
    set_error("rank: MHA with d_att %u and %u heads has no kernel", m->mh_datt, m->mh_heads);
    return PG_ERR_UNSUPPORTED;
}

// h_off: the call's offsets on the host, needed (to cut runs of at most kMhaRunReqs requests) only when n_req exceeds that
int rank_mha_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user, const uint32_t* d_seq_rows,
                        const uint32_t* d_seq_off, const uint32_t* d_cand, const uint32_t* d_off, const uint32_t* h_off,
                        uint32_t n_req, uint32_t n_items, float* d_out) {
    if (n_items == 0 || n_req == 0) return PG_OK;
    const int bf16 = m->prec == 1;
    const uint32_t cap = std::min(n_items, kDinRunItems), req_cap = std::min(n_req, kMhaRunReqs);
    const uint32_t max_tiles = cap / kBM + req_cap;
    const size_t rb = (size_t)mha_rec_bytes(bf16, (int)m->mh_datt);
    float* stage;
    uint32_t *ident, *loc_off, *tile_req, *tile_item0, *tile_cnt, *n_tiles, *req_tile0, *n_valid;
    char* kv;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotMha, [&](Carve& c) {
            stage = c.take<float>((size_t)cap * kDIN);
            ident = c.take<uint32_t>(cap);
            loc_off = c.take<uint32_t>((size_t)req_cap + 1);
            tile_req = c.take<uint32_t>(max_tiles);
            tile_item0 = c.take<uint32_t>(max_tiles);
            tile_cnt = c.take<uint32_t>(max_tiles);
            n_tiles = c.take<uint32_t>(64);
            req_tile0 = c.take<uint32_t>(req_cap);
            n_valid = c.take<uint32_t>(req_cap);
            kv = (char*)c.bytes((size_t)req_cap * kMhaMaxBlocks * rb);
        }))) return rc;
    pg_table staged;                    // the staging rows as the trunk's 128-wide table
    staged.d = stage;
    staged.rows = cap;
    staged.dim = kDIN;
    MhaKvArgs ka{};
    ka.loc_off = loc_off;
    ka.tab = t->d;
    ka.tab_rows = (uint32_t)t->rows;
    ka.seq_rows = d_seq_rows;
    ka.wk = m->mh_wk;
    ka.wv = m->mh_wv;
    ka.bv = m->mh_bv;
    ka.n_valid = n_valid;
    ka.kv = kv;
    MhaArgs a{};
    a.tile_req = tile_req;
    a.tile_item0 = tile_item0;
    a.tile_cnt = tile_cnt;
    a.n_tiles = n_tiles;
    a.tab = t->d;
    a.tab_rows = (uint32_t)t->rows;
    a.n_valid = n_valid;
    a.kv = kv;
    a.wq = (const char*)m->mh_wq;
    a.wo = (const char*)m->mh_wo;
    a.bq = m->mh_bq;
    a.stage = stage;
    // the rank timer spans the prologue, the attention and the trunk of every run: the trunk's own events stay off
    const bool timed = !ctx->timers_off;
    if (timed) PG_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    {
        TimersScope quiet(ctx, false);
        uint32_t r0 = 0;                // the run's first request (0 throughout when the call has at most kMhaRunReqs)
        for (uint32_t lo = 0; lo < n_items;) {
            uint32_t n = std::min(kDinRunItems, n_items - lo), nr = n_req;
            if (n_req > kMhaRunReqs) {
                while (h_off[r0 + 1] <= lo) ++r0;                     // the request that holds candidate lo
                nr = std::min(kMhaRunReqs, n_req - r0);
                n = std::min(n, h_off[r0 + nr] - lo);
            }
            din_run_launch(ctx, d_off + r0, nr, lo, lo + n, loc_off, ident);
            PG_HIP(hipGetLastError());
            if ((rc = build_tiles_launch(ctx, loc_off, nr, max_tiles, kBM, tile_req, tile_item0, tile_cnt, n_tiles, req_tile0))) return rc;
            ka.seq_off = d_seq_off + r0;
            a.cand_rows = d_cand + lo;
            const uint32_t grid = n / kBM + nr;
            if ((rc = bf16 ? launch_mha_shape<1>(ctx, m, ka, nr, a, grid) : launch_mha_shape<0>(ctx, m, ka, nr, a, grid))) return rc;
            if ((rc = rank_dnn3_dev_locked(ctx, m, &staged, d_user + (size_t)r0 * m->d_user, ident, loc_off, nr, n, d_out + lo, n_items))) return rc;
            lo += n;
        }
    }
    if (timed) {
        PG_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->rank_timing_pending = true;
    }
    return PG_OK;
}

}  // namespace pg
