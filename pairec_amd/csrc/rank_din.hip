// rank_din.hip — PG_MODEL_DIN: attention of every candidate over the request's behaviour sequence, in front of the DNN3 trunk.
//
// The reference loads a user's behaviour sequence as a first-class feature (Feature_Type_Sequence, module/feature_dao.go:19,
// 94-134; SequenceLength / SequenceName / SequenceEvent, recconf/recconf.go:202-212) and ships it to a remote DIN
// (TEST_TORCHREC_DIN_TOKEN, algorithm/eas/easyrec_predict_test.go).  Here the sequence is a list of rows of the item table the
// candidates come from, and the activation unit runs on the matrix pipe:
//     z_l = [e | s_l | e - s_l | e * s_l]      a_l = wa2 . relu(Wa' z_l + ba) + ba2      pooled = sum_l a_l s_l
//
// One GEMM per request.  rank_model.hpp folds Wa = [We; Ws; Wd; Wp] into Wq = We + Wd, Wk = Ws - Wd, so that
//     Wa' z_l = Wq' e + Wk' s_l + Wp' (e * s_l) = B_l' e + C0_l,   B_l[d][h] = s_l[d] Wp[d][h] + Wq[d][h],   C0_l = Wk' s_l + ba
// B and C0 depend on the request alone: every pre-activation of a tile is E[items x 64] . B[64 x (L att_h)] on accumulators
// that start at C0, and the per-pair operand e * s_l is never formed.
//
// Candidates on the MFMA column axis.  The kernel computes B' . E': a 32 x 32 accumulator block has rows (position, hidden
// unit) — one position with att_h = 32, two with 16 — and columns = items.  A lane then owns one item and 16 hidden units of
// it: relu, the wa2 dot product and ba2 run over the lane's own registers plus ONE exchange between the lane halves, and the
// pooling is a short loop per lane over s_l read from LDS at an address all lanes of a half share (a broadcast).
//
// Work split: one workgroup of 4 waves per tile of up to 128 candidates of one request (the trunk's tile builder), wave w the
// items 32 w .. 32 w + 31.  A lane reads its item's row straight from the table into MFMA operand registers — the whole row is
// used by the two lanes of an item, and it stays in registers for every position, so the rows never pass through LDS — and
// writes the fp32 values it read to the staging row.  The B operand is built in LDS a chunk of kDinCols = 256 columns at a
// time (Lc = 256 / att_h positions: 8 or 16), in MFMA fragment order (1 KiB per (block, k-group): reads are one conflict-free
// 16-B load per lane), every thread holding its 8 + 8 weights of Wp / Wq in registers across all positions.
//
// LDS per workgroup (of 160 KB per CU):  s rows 64 x 64 fp32 = 16 KB;  C0 64 x att_h fp32 = 4 / 8 KB;  B chunk 256 x 64:
// 32 KB in bf16, 64 KB in fp32.  BF16 form: 52 / 56 KB — two workgroups per CU, one building while the other multiplies.
// F32 form: 84 / 88 KB, one workgroup per CU.
//
// Two forms.  F32 (PG_PREC_F32, and in front of the split-bf16 trunk of PG_PREC_BF16X3): v_mfma_f32_32x32x2_f32, nothing
// rounded.  BF16: v_mfma_f32_32x32x16_bf16; candidate rows and B are each rounded once (RNE) from their fp32 values; C0, the
// accumulation, relu, the wa2 reduction, a_l and the pooling stay fp32.
//
// Masking: positions l >= L are never visited (L = min(sequence length, PG_DIN_MAX_SEQ)); a sequence row at or past the
// table's row count is a zero row for which nothing is read (a_l . 0 adds nothing); candidate rows past the table clamp to
// the last row as in the DNN3 gather; L = 0 writes pooled = 0.
//
// Output: [e | pooled], 128 fp32 per candidate, into the staging rows of kSlotDin; rank_dnn3_dev_locked then runs the
// unchanged trunk over them as a 128-wide table with an identity candidate list.
#include "rank_mlp.hpp"

#include <algorithm>

namespace pg {

constexpr int kDinCols = 256;       // (position, hidden unit) columns of one B chunk

struct DinArgs {
    const uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles;   // tiles over the run's own offsets
    const float* tab;
    uint32_t tab_rows;
    const uint32_t* cand_rows;      // the run's first candidate
    const uint32_t* seq_rows;
    const uint32_t* seq_off;
    const float *wq, *wk, *wp, *ba, *wa2;
    float ba2;
    float* stage;                   // [run items][kDIN]
};

constexpr size_t din_lds_bytes(int bf16, int att_h) {
    return (size_t)PG_DIN_MAX_SEQ * kDinD * 4 + (size_t)PG_DIN_MAX_SEQ * att_h * 4 + (size_t)kDinCols * kDinD * (bf16 ? 2 : 4);
}

template <int BF16, int ATT_H>
__global__ __launch_bounds__(256) void din_attn_kernel(DinArgs a) {
    constexpr int D = kDinD;
    constexpr int LC = kDinCols / ATT_H;          // positions per chunk
    constexpr int POSB = 32 / ATT_H;              // positions per 32-row accumulator block
    constexpr int NBLK = kDinCols / 32;           // blocks per chunk
    constexpr int KF = BF16 ? D / 16 : D / 8;     // 1-KiB fragments per block (k-groups of the 64-deep product)
    constexpr int NG = 256 / ATT_H;               // C0: positions computed side by side
    constexpr int NPOS = PG_DIN_MAX_SEQ / NG;     // C0: positions per thread
    constexpr int RPP = 16 / POSB;                // accumulator registers per position
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    static_assert(ATT_H == 16 || ATT_H == 32, "attention width");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const S = reinterpret_cast<float*>(smem);                  // [64][64] sequence rows
    float* const C0 = S + PG_DIN_MAX_SEQ * D;                         // [64][ATT_H]
    char* const BT = reinterpret_cast<char*>(C0 + PG_DIN_MAX_SEQ * ATT_H);   // [NBLK][KF] fragments

    const uint32_t tile = blockIdx.x;
    if (tile >= *a.n_tiles) return;
    const uint32_t req = a.tile_req[tile];
    const uint32_t item0 = a.tile_item0[tile];
    const uint32_t cnt = a.tile_cnt[tile];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hk = lane >> 5;
    const uint32_t s0 = a.seq_off[req], s1 = a.seq_off[req + 1];
    const int L = s1 > s0 ? (s1 - s0 < (uint32_t)PG_DIN_MAX_SEQ ? (int)(s1 - s0) : PG_DIN_MAX_SEQ) : 0;
    const int Lpad = (L + POSB - 1) / POSB * POSB;                    // a block's second position may lie past L: a zero row

    // ---- the sequence rows into LDS: 16 lanes x 16 B per row --------------------------------------------------------------
    for (int l = tid >> 4; l < Lpad; l += 16) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l < L) {
            const uint32_t row = a.seq_rows[s0 + l];
            if (row < a.tab_rows) v = *reinterpret_cast<const float4*>(a.tab + (size_t)row * D + 4 * (tid & 15));
        }
        *reinterpret_cast<float4*>(S + l * D + 4 * (tid & 15)) = v;
    }

    // ---- this lane's item: its row as MFMA operand registers, the fp32 values on to the staging row ------------------------
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
            u32x4 p;
            p.x = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v0.x, v0.y}, bf16x2));   // v_cvt_pk_bf16_f32 (RNE)
            p.y = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v0.z, v0.w}, bf16x2));
            p.z = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v1.x, v1.y}, bf16x2));
            p.w = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v1.z, v1.w}, bf16x2));
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

    // ---- the builder's weights: thread (i, q, sp) makes rows 8 q .. 8 q + 7 of column (position = sp mod POSB, unit i) ------
    const int bi = tid % ATT_H, bq = (tid / ATT_H) & 7, bsp = tid / (ATT_H * 8);
    float wpr[8], wqr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        wpr[e] = a.wp[(8 * bq + e) * ATT_H + bi];
        wqr[e] = a.wq[(8 * bq + e) * ATT_H + bi];
    }
    // the lane's 16 hidden units: register r of a block is row (r & 3) + 8 (r >> 2) + 4 hk
    float w2r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) w2r[r] = a.wa2[((r & 3) + 8 * (r >> 2) + 4 * hk) % ATT_H];
    __syncthreads();                                                  // S complete

    // ---- C0[l][h] = ba[h] + sum_d Wk[d][h] s_l[d], d ascending: a thread keeps half a column of Wk and walks its positions ---
    {
        const int h = tid % ATT_H, lg = tid / ATT_H;
        float c0[NPOS];
        const float bah = a.ba[h];
#pragma unroll
        for (int p = 0; p < NPOS; ++p) c0[p] = bah;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float wk[D / 2];
#pragma unroll
            for (int d = 0; d < D / 2; ++d) wk[d] = a.wk[(half * (D / 2) + d) * ATT_H + h];
#pragma unroll
            for (int p = 0; p < NPOS; ++p) {
                const int l = lg + p * NG;
                if (l < Lpad) {
#pragma unroll
                    for (int d4 = 0; d4 < D / 8; ++d4) {
                        const float4 sv = *reinterpret_cast<const float4*>(S + l * D + half * (D / 2) + 4 * d4);
                        c0[p] = __fmaf_rn(wk[4 * d4 + 0], sv.x, c0[p]);
                        c0[p] = __fmaf_rn(wk[4 * d4 + 1], sv.y, c0[p]);
                        c0[p] = __fmaf_rn(wk[4 * d4 + 2], sv.z, c0[p]);
                        c0[p] = __fmaf_rn(wk[4 * d4 + 3], sv.w, c0[p]);
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NPOS; ++p) {
            const int l = lg + p * NG;
            if (l < Lpad) C0[l * ATT_H + h] = c0[p];
        }
    }

    float pooled[D / 2];                // lane (j, hk): pooled[32 hk + 0..31] of item j
#pragma unroll
    for (int d = 0; d < D / 2; ++d) pooled[d] = 0.f;

    for (int l0 = 0; l0 < L; l0 += LC) {
        const int nblk = (Lpad - l0) / POSB < NBLK ? (Lpad - l0) / POSB : NBLK;
        __syncthreads();                // C0 complete; the chunk before this one has been read
        // ---- B of the chunk, in fragment order ----
        for (int b = 0; b < nblk; ++b) {
            const int l = l0 + b * POSB + bsp;
            const float4 sa = *reinterpret_cast<const float4*>(S + l * D + 8 * bq);
            const float4 sb = *reinterpret_cast<const float4*>(S + l * D + 8 * bq + 4);
            const float v[8] = {__fmaf_rn(sa.x, wpr[0], wqr[0]), __fmaf_rn(sa.y, wpr[1], wqr[1]), __fmaf_rn(sa.z, wpr[2], wqr[2]),
                                __fmaf_rn(sa.w, wpr[3], wqr[3]), __fmaf_rn(sb.x, wpr[4], wqr[4]), __fmaf_rn(sb.y, wpr[5], wqr[5]),
                                __fmaf_rn(sb.z, wpr[6], wqr[6]), __fmaf_rn(sb.w, wpr[7], wqr[7])};
            const int ri = bsp * ATT_H + bi;                          // row of the block
            if constexpr (BF16) {
                // fragment (b, ks): lane (ri, hk') holds B[16 ks + 8 hk' + 0..7][ri]; this thread's 8 rows are ks = q / 2, hk' = q & 1
                u32x4 p;
                p.x = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v[0], v[1]}, bf16x2));
                p.y = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v[2], v[3]}, bf16x2));
                p.z = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v[4], v[5]}, bf16x2));
                p.w = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v[6], v[7]}, bf16x2));
                *reinterpret_cast<u32x4*>(BT + (b * KF + (bq >> 1)) * 1024 + ((bq & 1) * 32 + ri) * 16) = p;
            } else {
                // fragment (b, g8 = q): lane (ri, hh) holds B[8 q + 2 st + hh][ri], st = 0..3
                char* const f = BT + (b * KF + bq) * 1024 + ri * 16;
                *reinterpret_cast<float4*>(f) = make_float4(v[0], v[2], v[4], v[6]);
                *reinterpret_cast<float4*>(f + 512) = make_float4(v[1], v[3], v[5], v[7]);
            }
        }
        __syncthreads();
        if ((uint32_t)wave * 32 >= cnt) continue;                     // (wave-uniform; the barriers above are taken by every wave)
        // ---- pre-activations of the wave's 32 items against the chunk, a block at a time ----
        for (int b = 0; b < nblk; ++b) {
            f32x16 acc;
            const float* const c0p = C0 + (l0 + b * POSB) * ATT_H + 4 * hk;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const float4 c = *reinterpret_cast<const float4*>(c0p + 8 * qd);
                acc[4 * qd + 0] = c.x; acc[4 * qd + 1] = c.y; acc[4 * qd + 2] = c.z; acc[4 * qd + 3] = c.w;
            }
            if constexpr (BF16) {
#pragma unroll
                for (int ks = 0; ks < KF; ++ks) {
                    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(BT + (b * KF + ks) * 1024 + lane * 16);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf, eb[ks], acc, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int g8 = 0; g8 < KF; ++g8) {
                    const f32x4 bf = *reinterpret_cast<const f32x4*>(BT + (b * KF + g8) * 1024 + lane * 16);
#pragma unroll
                    for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[st], ef[g8 * 4 + st], acc, 0, 0, 0);
                }
            }
            // ---- a_l = ba2 + sum_h wa2[h] relu(.) over the lane's registers and its partner's; pooled += a_l s_l ----
#pragma unroll
            for (int sp = 0; sp < POSB; ++sp) {
                float v = 0.f;
#pragma unroll
                for (int r = sp * RPP; r < (sp + 1) * RPP; ++r) v = __fmaf_rn(w2r[r], fmaxf(acc[r], 0.f), v);
                v = v + __shfl_xor(v, 32);
                const float al = v + a.ba2;
                const float* const sl = S + (l0 + b * POSB + sp) * D + 32 * hk;
#pragma unroll
                for (int c = 0; c < D / 8; ++c) {
                    const float4 sv = *reinterpret_cast<const float4*>(sl + 4 * c);
                    pooled[4 * c + 0] = __fmaf_rn(al, sv.x, pooled[4 * c + 0]);
                    pooled[4 * c + 1] = __fmaf_rn(al, sv.y, pooled[4 * c + 1]);
                    pooled[4 * c + 2] = __fmaf_rn(al, sv.z, pooled[4 * c + 2]);
                    pooled[4 * c + 3] = __fmaf_rn(al, sv.w, pooled[4 * c + 3]);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < D / 8; ++c)
            *reinterpret_cast<float4*>(out_row + D + 32 * hk + 4 * c) =
                make_float4(pooled[4 * c], pooled[4 * c + 1], pooled[4 * c + 2], pooled[4 * c + 3]);
    }
}

// a run's own offsets (the call's, clamped to the run's candidates [lo, hi) and rebased) and the identity candidate list
__global__ void din_run_kernel(const uint32_t* __restrict__ off, uint32_t n_req, uint32_t lo, uint32_t hi, uint32_t* __restrict__ loc_off,
                               uint32_t* __restrict__ ident) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_req) {
        const uint32_t o = off[i];
        loc_off[i] = (o < lo ? lo : (o > hi ? hi : o)) - lo;
    }
    if (i < hi - lo) ident[i] = i;
}

void din_run_launch(pg_ctx* ctx, const uint32_t* d_off, uint32_t n_req, uint32_t lo, uint32_t hi, uint32_t* loc_off, uint32_t* ident) {
    din_run_kernel<<<(std::max(hi - lo, n_req + 1) + 255) / 256, 256, 0, ctx->stream>>>(d_off, n_req, lo, hi, loc_off, ident);
}

template <int BF16, int ATT_H>
static int launch_din_attn(pg_ctx* ctx, const DinArgs& a, uint32_t grid) {
    constexpr size_t lds = din_lds_bytes(BF16, ATT_H);
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)din_attn_kernel<BF16, ATT_H>, lds))) return rc;
    din_attn_kernel<BF16, ATT_H><<<grid, 256, lds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int rank_din_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user, const uint32_t* d_seq_rows,
                        const uint32_t* d_seq_off, const uint32_t* d_cand, const uint32_t* d_off, uint32_t n_req, uint32_t n_items,
                        float* d_out) {
    if (n_items == 0 || n_req == 0) return PG_OK;
    const uint32_t cap = std::min(n_items, kDinRunItems);
    const uint32_t max_tiles = cap / kBM + n_req;
    float* stage;
    uint32_t *ident, *loc_off, *tile_req, *tile_item0, *tile_cnt, *n_tiles, *req_tile0;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotDin, [&](Carve& c) {
            stage = c.take<float>((size_t)cap * kDIN);
            ident = c.take<uint32_t>(cap);
            loc_off = c.take<uint32_t>((size_t)n_req + 1);
            tile_req = c.take<uint32_t>(max_tiles);
            tile_item0 = c.take<uint32_t>(max_tiles);
            tile_cnt = c.take<uint32_t>(max_tiles);
            n_tiles = c.take<uint32_t>(64);
            req_tile0 = c.take<uint32_t>(n_req);
        }))) return rc;
    pg_table staged;                    // the staging rows as the trunk's 128-wide table
    staged.d = stage;
    staged.rows = cap;
    staged.dim = kDIN;
    DinArgs a{};
    a.tile_req = tile_req;
    a.tile_item0 = tile_item0;
    a.tile_cnt = tile_cnt;
    a.n_tiles = n_tiles;
    a.tab = t->d;
    a.tab_rows = (uint32_t)t->rows;
    a.seq_rows = d_seq_rows;
    a.seq_off = d_seq_off;
    a.wq = m->att_wq;
    a.wk = m->att_wk;
    a.wp = m->att_wp;
    a.ba = m->att_ba;
    a.wa2 = m->att_wa2;
    a.ba2 = m->att_ba2;
    a.stage = stage;
    // the rank timer spans the attention and the trunk of every run: the trunk's own events stay off
    const bool timed = !ctx->timers_off;
    if (timed) PG_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    {
        TimersScope quiet(ctx, false);
        for (uint32_t lo = 0; lo < n_items; lo += kDinRunItems) {
            const uint32_t n = std::min(kDinRunItems, n_items - lo);
            din_run_launch(ctx, d_off, n_req, lo, lo + n, loc_off, ident);
            PG_HIP(hipGetLastError());
            if ((rc = build_tiles_launch(ctx, loc_off, n_req, max_tiles, kBM, tile_req, tile_item0, tile_cnt, n_tiles, req_tile0))) return rc;
            a.cand_rows = d_cand + lo;
            const uint32_t grid = n / kBM + n_req;
            if (m->prec == 1) rc = m->att_h == 32 ? launch_din_attn<1, 32>(ctx, a, grid) : launch_din_attn<1, 16>(ctx, a, grid);
            else rc = m->att_h == 32 ? launch_din_attn<0, 32>(ctx, a, grid) : launch_din_attn<0, 16>(ctx, a, grid);
            if (rc) return rc;
            if ((rc = rank_dnn3_dev_locked(ctx, m, &staged, d_user, ident, loc_off, n_req, n, d_out + lo, n_items))) return rc;
        }
    }
    if (timed) {
        PG_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->rank_timing_pending = true;
    }
    return PG_OK;
}

}  // namespace pg
