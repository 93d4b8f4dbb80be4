// rank_ple.hip — PG_MODEL_PLE: progressive layered extraction (Tang et al., RecSys 2020), one or two levels of task and shared
// experts under task towers, a candidate's whole forward pass in registers.
//
// Groups g = 0 .. T: group t < T belongs to task t (E_t experts), group T is shared (E_s experts).  Level l, x0_g = x = [u | e]:
//     a_{g,k} = relu(We_{g,k}' x^{l-1}_g + be_{g,k})
//     task t:  x^l_t = sum softmax(Wg_t' x^{l-1}_t + bg_t)[k] a_k   over its own experts, then the shared ones
//     shared:  x^l_T = the same over every group's experts          (below the last level only)
//     score_t = sigmoid(wo_t . relu(Wt_t' x^{last}_t + bt_t) + bo_t)
// This is not rank_mmoe.hip's data flow: a gate mixes a subset of the experts, and the second level's T + 1 groups read T + 1
// different inputs that exist only once the whole first level is done.
//
// Work split as rank_mmoe.hip: one workgroup of 4 waves per tile of up to 128 candidates of one request, candidates on the MFMA
// column axis, lane (j, hk) of wave w item 32 w + j, its table row read straight into B-operand registers.  Group positions are
// fixed — task t at t, the shared group at 3 — so every register array is indexed at compile time while T, E_t and E_s are
// run-time values: a missing task's code is skipped by a wave-uniform branch, a missing second expert is a zero row with gate 0.
//
// Level 1.  The user half of every row (the 32 gate rows and every expert row) comes once per request from
// mmoe_user_partial_launch; the item half is one d_item-deep product from the lane's row registers.  The gate block holds the task
// gates in half 0 (slot 4 t + c) and the shared gate in half 1 (slots 0..7), so each softmax (max-subtracted, expf, rows of
// experts the model lacks masked out) runs over a lane's own registers and one exchange hands every lane all 12 + 8 gates.  An
// expert block is one GROUP: slot 8 k + u of half hk is (expert k, hidden unit 16 s + 8 hk + u), so after a step's blocks a lane
// holds, for its 8 hidden units, every expert that any gate mixes, and all T + 1 mixes run over its own registers.  The shared
// block comes first in a step and stays; task t's block is mixed as soon as it is done (own + shared) and adds its share to the
// shared mix, so only two blocks are live.
//
// Between the levels nothing leaves the lane.  The 8 mixed values of (group g, step s) are exactly the 8 k-values the lane
// supplies for slice s of group g's 64-deep second-level product: they are converted (BF16) or split (BF16X3) once into
// x1[g][s] — (T + 1) x 4 x 4 packed registers per part, 128 in BF16X3 — while the candidate-row registers die with level 1.
// The second level's task-gate logits are NOT products of those operands: they are fp32 fma chains over the mixed values (the
// unrounded ones in BF16X3, the rounded ones in BF16) against plain fp32 gate weights in LDS, each lane over its 8 units per
// step, the two halves added by one exchange at the end.  A logit is an exponent; a two-way split leaves 2^-18 of it.  For the
// same reason level 1's EXPERTS take the gate block's three-way split (three planes, six products) in a two-level BF16X3 model:
// level 2's gates exponentiate what those experts produce, and the 2^-18 that three products leave of x1 showed as 2.94e-7 of a
// score under +-80 logits (bar 2.83e-7; an fp64 evaluation with only that split applied: 3.01e-7).  One-level models and level 2's
// own experts keep three products: nothing exponentiates their outputs.
//
// Level 2 is block-structured: group g's block (s2, g) reads only x1[g][0..3].  Per step the shared block, then task t's block,
// task t's mix under its second-level gates, and the mix straight into the tower MFMAs of slice s2 — as MMoE's.  With one level
// the first level's task mixes feed the towers the same way and neither the shared gate nor x1 exists.
//
// LDS holds weights only: the gate record (and the second level's gate weights, 3 KB), then two buffers for the host-packed
// records (rank_model.hpp: pack_ple) — one record per (step, group), of one size per level, the last level's task records
// carrying the tower fragments of their slice.  The next record is requested from global memory before a block's MFMAs and
// written to the other buffer after them, one barrier per record.  Largest: d_item 128, two levels, BF16X3: 27 + 2 x 24 = 75 KB
// (one level, h_t 64: 24 + 2 x 20 = 64 KB), so no shape is single-buffered.
//
// Instantiations: <NP, d_item, levels, h_t> = 16; T, E_t, E_s and (with one level) h_e are run-time.
#include "rank_mlp.hpp"

#include <type_traits>

namespace pg {

struct PleArgs {
    const uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles;
    const float* tab;
    uint32_t tab_rows;
    const uint32_t* cand_rows;
    const float* c1;            // [n_req][nc]
    uint32_t nc;                // 32 + 32 records of level 1
    uint32_t steps;             // h_e / 16
    uint32_t n_task, task_mask, shared_mask;
    const char* rec;            // the gate record, then the records
    const float *be2, *bg2;     // level 2: [records][32] expert biases, [3][4] task-gate biases
    const float *bt, *wo, *bo;  // [3][h_t], [3][h_t], [3]
    float* out;
    size_t out_stride;
};

// softmax over v[0..N-1] in place, max-subtracted; a slot outside `mask` gets weight 0
template <int N>
__device__ __forceinline__ void ple_softmax(float* v, uint32_t mask) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if ((mask >> k) & 1) mx = fmaxf(mx, v[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        v[k] = (mask >> k) & 1 ? expf(v[k] - mx) : 0.f;
        sum = sum + v[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] / sum;
}

// one expert block: bias (the lane's 16 rows at `bias`), then NK 16-deep slices of B = bh (+ bl (+ b3)) against the fragments at `cur`
// (PL planes each: 1, 2 = three products, 3 = six), relu
template <int PL, int NK>
__device__ __forceinline__ f32x16 ple_block(const char* cur, int lane, const bf16x8* bh, const bf16x8* bl, const bf16x8* b3, const float* bias) {
    f32x16 acc = mmoe_rows16(bias);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        if constexpr (PL == 3)
            acc = mmoe_mac6(cur + ks * 3072, lane, bh[ks], bl[ks], b3[ks], acc);
        else
            acc = mmoe_mac<PL == 2 ? 3 : 1>(cur + ks * PL * 1024, lane, bh[ks], bl[PL == 2 ? ks : 0], acc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.f);
    return acc;
}

// a task's mix of its own block and the shared block under its four gates (own 0, own 1, shared 0, shared 1), in that order
__device__ __forceinline__ void ple_task_mix(const float* g, const f32x16& own, const f32x16& sh, float* mv) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float v = g[0] * own[u];
        v = __fmaf_rn(g[1], own[8 + u], v);
        v = __fmaf_rn(g[2], sh[u], v);
        mv[u] = __fmaf_rn(g[3], sh[8 + u], v);
    }
}

template <int NP, int D, int NL, int HT>
__global__ __launch_bounds__(256) void ple_kernel(PleArgs a) {
    constexpr int KS = D / 16;                  // k-groups of the d_item-deep product
    constexpr int HB = HT / 32;                 // blocks of a tower
    constexpr int FRAG = (NP == 3 ? 2 : 1) * 1024;
    constexpr int GFRAG = (NP == 3 ? 3 : 1) * 1024;
    constexpr int PREC = NP == 3 ? 2 : 1;
    constexpr int P1 = (int)ple_l1_planes(NL, PREC);    // planes of level 1's expert fragments: 3 in split bf16 under a second level
    constexpr int GBYTES = (int)ple_gate_bytes(D, NL, PREC);
    constexpr int RB1 = (int)ple_rec1_bytes(D, NL, HT, PREC), RB2 = NL == 2 ? (int)ple_rec2_bytes(HT, PREC) : 0;     // a record of level 1, of level 2
    constexpr int RBYTES = RB1 > RB2 ? RB1 : RB2;       // a buffer
    constexpr int NLD = (RBYTES / 16 + 255) / 256;      // 16-B loads per thread and record
    constexpr int XG = NL == 2 ? 4 : 1, XS = NL == 2 ? 4 : 1, XL = NL == 2 && NP == 3 ? 4 : 1;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    static_assert((NL == 1 || NL == 2) && (HT == 32 || HT == 64) && (D == 64 || D == 128), "shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const GT = smem;                      // the gate record
    const float4* const WG2 = reinterpret_cast<const float4*>(smem + KS * GFRAG);       // level 2's task gates [3][64]
    char* const BUF = smem + GBYTES;            // two records

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
    const char* const recs = a.rec + GBYTES;
    const uint32_t T = a.n_task, n_rec1 = a.steps * (T + 1), n_rec = n_rec1 * NL;

    // ---- the gate record and record 0 into LDS -----------------------------------------------------------------------------
    for (int i = tid; i < GBYTES / 16; i += 256) reinterpret_cast<u32x4*>(GT)[i] = reinterpret_cast<const u32x4*>(a.rec)[i];
    for (int i = tid; i < RB1 / 16; i += 256) reinterpret_cast<u32x4*>(BUF)[i] = reinterpret_cast<const u32x4*>(recs)[i];

    // ---- this lane's item: its row as B-operand registers ------------------------------------------------------------------
    const uint32_t r_item = wave * 32 + j;
    const bool live = r_item < cnt;
    uint32_t erow = a.cand_rows[item0 + (live ? r_item : cnt - 1)];
    erow = erow < a.tab_rows ? erow : a.tab_rows - 1;
    const float4* const ep = reinterpret_cast<const float4*>(a.tab + (size_t)erow * D);
    bf16x8 eh[KS], el[NP == 3 ? KS : 1], e3[NP == 3 ? KS : 1];     // (e3: the third part, for the gate block and the three-plane experts)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const float4 v0 = ep[ks * 4 + 2 * hk], v1 = ep[ks * 4 + 2 * hk + 1];
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        mmoe_operand<NP>(v, eh[ks], el[NP == 3 ? ks : 0]);
        if constexpr (NP == 3) {
            float rest[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) rest[i] = (v[i] - (float)eh[ks][i]) - (float)el[ks][i];      // (both exact)
            bf16x8 unused;
            mmoe_operand<1>(rest, e3[ks], unused);
        }
    }
    const float* const c1r = a.c1 + (size_t)req * a.nc + 4 * hk;
    __syncthreads();

    // ---- level 1's gates: one block, every softmax over the lane's own registers, one exchange between the halves ----------
    float g1[3][4], gs[8];
    f32x16 at[3 * HB];
    if (active) {
        f32x16 ga = mmoe_rows16(c1r);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if constexpr (NP == 3)
                ga = mmoe_mac6(GT + ks * GFRAG, lane, eh[ks], el[ks], e3[ks], ga);
            else
                ga = mmoe_mac<1>(GT + ks * GFRAG, lane, eh[ks], el[0], ga);
        }
        // half 0 holds the task logits, half 1 the shared ones: both forms are computed and the half that holds garbage is not read
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            float v[4] = {ga[4 * t], ga[4 * t + 1], ga[4 * t + 2], ga[4 * t + 3]};
            ple_softmax<4>(v, a.task_mask);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float o = __shfl_xor(v[c], 32);
                g1[t][c] = hk == 0 ? v[c] : o;
            }
        }
        if constexpr (NL == 2) {
#pragma unroll
            for (int k = 0; k < 8; ++k) gs[k] = ga[k];
            ple_softmax<8>(gs, a.shared_mask);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float o = __shfl_xor(gs[k], 32);
                gs[k] = hk == 1 ? gs[k] : o;
            }
        }
#pragma unroll
        for (int tb = 0; tb < 3 * HB; ++tb) at[tb] = mmoe_rows16(a.bt + tb * 32 + 4 * hk);
    }

    // ---- the record pipeline: stage ri reads buffer ri & 1 while record ri + 1 travels to the other ------------------------
    uint32_t ri = 0;
    u32x4 pre[NLD];
    auto request = [&]() __attribute__((always_inline)) {
        if (ri + 1 < n_rec) {
            const bool l2 = ri + 1 >= n_rec1;       // (level 1's records, then level 2's: two sizes)
            const u32x4* const next = reinterpret_cast<const u32x4*>(recs + (l2 ? (size_t)n_rec1 * RB1 + (size_t)(ri + 1 - n_rec1) * RB2 : (size_t)(ri + 1) * RB1));
            const int n16 = (l2 ? RB2 : RB1) / 16;
#pragma unroll
            for (int c = 0; c < NLD; ++c)
                if (tid + 256 * c < n16) pre[c] = next[tid + 256 * c];
        }
    };
    auto deliver = [&]() __attribute__((always_inline)) {
        if (ri + 1 < n_rec) {
            u32x4* const dst = reinterpret_cast<u32x4*>(BUF + ((ri + 1) & 1) * RBYTES);       // last read in stage ri - 1
            const int n16 = (ri + 1 >= n_rec1 ? RB2 : RB1) / 16;
#pragma unroll
            for (int c = 0; c < NLD; ++c)
                if (tid + 256 * c < n16) dst[tid + 256 * c] = pre[c];
        }
        __syncthreads();
        ++ri;
    };
    // the tower MFMAs of one 16-deep slice of task t: the mix as the B operand against the fragments behind the block's
    auto towers = [&](int t, const float* mv, const char* frags) __attribute__((always_inline)) {
        bf16x8 mh, ml;
        mmoe_operand<NP>(mv, mh, ml);
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) at[t * HB + hb] = mmoe_mac<NP>(frags + hb * FRAG, lane, mh, ml, at[t * HB + hb]);
    };

    bf16x8 x1h[XG][XS], x1l[XG][XL];            // level 2's B operands: [group position][slice]
    float z2[3][4];                             // level 2's task-gate logits, this half's share
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) z2[t][c] = 0.f;

    // ---- level 1 in steps of 16 hidden units: the shared block, then each task's block and its mix -------------------------
    auto level1_step = [&](auto s_static, uint32_t s) __attribute__((always_inline)) {
        constexpr int SS = decltype(s_static)::value;       // the slice of x1 this step fills (two levels: the loop is unrolled)
        f32x16 sh;
        float ms[8];
        request();
        if (active) {
            sh = ple_block<P1, KS>(BUF + (ri & 1) * RBYTES, lane, eh, el, e3, c1r + 32 + ri * 32);
            if constexpr (NL == 2) {
#pragma unroll
                for (int u = 0; u < 8; ++u) ms[u] = __fmaf_rn(gs[7], sh[8 + u], gs[6] * sh[u]);
            }
        }
        deliver();
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if ((uint32_t)t >= T) continue;
            request();
            if (active) {
                const char* const cur = BUF + (ri & 1) * RBYTES;
                const f32x16 own = ple_block<P1, KS>(cur, lane, eh, el, e3, c1r + 32 + ri * 32);
                float mv[8];
                ple_task_mix(g1[t], own, sh, mv);
                if constexpr (NL == 1) {
                    towers(t, mv, cur + KS * FRAG);
                } else {
                    mmoe_operand<NP>(mv, x1h[t][SS], x1l[t][NP == 3 ? SS : 0]);
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        ms[u] = __fmaf_rn(gs[2 * t + 1], own[8 + u], __fmaf_rn(gs[2 * t], own[u], ms[u]));
                        const float xv = NP == 3 ? mv[u] : (float)x1h[t][SS][u];
                        const float4 w = WG2[t * 64 + 16 * s + 8 * hk + u];
                        z2[t][0] = __fmaf_rn(w.x, xv, z2[t][0]);
                        z2[t][1] = __fmaf_rn(w.y, xv, z2[t][1]);
                        z2[t][2] = __fmaf_rn(w.z, xv, z2[t][2]);
                        z2[t][3] = __fmaf_rn(w.w, xv, z2[t][3]);
                    }
                }
            }
            deliver();
        }
        if constexpr (NL == 2) {
            if (active) mmoe_operand<NP>(ms, x1h[3][SS], x1l[3][NP == 3 ? SS : 0]);
        }
    };
    if constexpr (NL == 1) {
        for (uint32_t s = 0; s < a.steps; ++s) level1_step(std::integral_constant<int, 0>{}, s);
    } else {
        level1_step(std::integral_constant<int, 0>{}, 0);
        level1_step(std::integral_constant<int, 1>{}, 1);
        level1_step(std::integral_constant<int, 2>{}, 2);
        level1_step(std::integral_constant<int, 3>{}, 3);

        // ---- level 2: its gates from the chains, then per step the shared block, each task's block, mix and tower slice ----
        float g2[3][4];
        if (active) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
#pragma unroll
                for (int c = 0; c < 4; ++c) g2[t][c] = (z2[t][c] + __shfl_xor(z2[t][c], 32)) + a.bg2[t * 4 + c];
                ple_softmax<4>(g2[t], a.task_mask);
            }
        }
        for (uint32_t s = 0; s < 4; ++s) {
            f32x16 sh;
            request();
            if (active) sh = ple_block<PREC, 4>(BUF + (ri & 1) * RBYTES, lane, x1h[3], x1l[3], nullptr, a.be2 + (size_t)(ri - n_rec1) * 32 + 4 * hk);
            deliver();
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                if ((uint32_t)t >= T) continue;
                request();
                if (active) {
                    const char* const cur = BUF + (ri & 1) * RBYTES;
                    const f32x16 own = ple_block<PREC, 4>(cur, lane, x1h[t], x1l[t], nullptr, a.be2 + (size_t)(ri - n_rec1) * 32 + 4 * hk);
                    float mv[8];
                    ple_task_mix(g2[t], own, sh, mv);
                    towers(t, mv, cur + 4 * FRAG);
                }
                deliver();
            }
        }
    }
    if (!active) return;

    // ---- the towers' heads: relu, the wo dot over the lane's rows and its partner's, bo, sigmoid ----------------------------
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if ((uint32_t)t >= T) continue;
        float v = 0.f;
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            const f32x16 w = mmoe_rows16(a.wo + (t * HB + hb) * 32 + 4 * hk);
#pragma unroll
            for (int r = 0; r < 16; ++r) v = __fmaf_rn(w[r], fmaxf(at[t * HB + hb][r], 0.f), v);
        }
        v = v + __shfl_xor(v, 32);
        const float z = v + a.bo[t];
        if (live && hk == 0) a.out[(size_t)t * a.out_stride + item0 + r_item] = 1.0f / (1.0f + expf(-z));
    }
}

template <int NP, int D, int NL, int HT>
static int launch_ple(pg_ctx* ctx, const PleArgs& a, uint32_t grid) {
    constexpr int prec = NP == 3 ? 2 : 1;
    constexpr size_t rb1 = ple_rec1_bytes(D, NL, HT, prec), rb2 = NL == 2 ? ple_rec2_bytes(HT, prec) : 0;
    constexpr size_t lds = ple_gate_bytes(D, NL, prec) + 2 * (rb1 > rb2 ? rb1 : rb2);
    static_assert(lds <= 128 * 1024, "LDS");
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)ple_kernel<NP, D, NL, HT>, lds))) return rc;
    ple_kernel<NP, D, NL, HT><<<grid, 256, lds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
template <int NP, int D>
static int launch_ple_shape(pg_ctx* ctx, const pg_model* m, const PleArgs& a, uint32_t grid) {
    if (m->n_level == 1) return m->h_t == 32 ? launch_ple<NP, D, 1, 32>(ctx, a, grid) : launch_ple<NP, D, 1, 64>(ctx, a, grid);
    return m->h_t == 32 ? launch_ple<NP, D, 2, 32>(ctx, a, grid) : launch_ple<NP, D, 2, 64>(ctx, a, grid);
}

int rank_ple_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user, const uint32_t* d_cand,
                        const uint32_t* d_off, uint32_t n_req, uint32_t n_items, float* d_out) {
    if (n_items == 0 || n_req == 0) return PG_OK;
    const uint32_t max_tiles = n_items / kBM + n_req, nc = 32 + 32 * m->pl_nrec1;
    float* c1;
    uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles, *req_tile0;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotPle, [&](Carve& c) {
            tile_req = c.take<uint32_t>(max_tiles);
            tile_item0 = c.take<uint32_t>(max_tiles);
            tile_cnt = c.take<uint32_t>(max_tiles);
            n_tiles = c.take<uint32_t>(64);
            req_tile0 = c.take<uint32_t>(n_req);
            c1 = c.take<float>((size_t)n_req * nc);
        }))) return rc;
    const bool timed = !ctx->timers_off;
    if (timed) PG_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((rc = build_tiles_launch(ctx, d_off, n_req, max_tiles, kBM, tile_req, tile_item0, tile_cnt, n_tiles, req_tile0))) return rc;
    if ((rc = mmoe_user_partial_launch(ctx, d_user, n_req, m->d_user, m->mm_wu, m->mm_bu, nc, c1))) return rc;
    PleArgs a{};
    a.tile_req = tile_req;
    a.tile_item0 = tile_item0;
    a.tile_cnt = tile_cnt;
    a.n_tiles = n_tiles;
    a.tab = t->d;
    a.tab_rows = (uint32_t)t->rows;
    a.cand_rows = d_cand;
    a.c1 = c1;
    a.nc = nc;
    a.steps = m->h_e / 16;
    a.n_task = m->n_out;
    a.task_mask = ple_task_mask(m->e_task, m->e_shared);
    a.shared_mask = ple_shared_mask(m->n_out, m->e_task, m->e_shared);
    a.rec = (const char*)m->mm_rec;
    a.be2 = m->pl_be2;
    a.bg2 = m->pl_bg2;
    a.bt = m->mm_bt;
    a.wo = m->mm_wo;
    a.bo = m->mm_bo;
    a.out = d_out;
    a.out_stride = n_items;
    if (m->prec == 2)
        rc = m->d_item == 64 ? launch_ple_shape<3, 64>(ctx, m, a, max_tiles) : launch_ple_shape<3, 128>(ctx, m, a, max_tiles);
    else
        rc = m->d_item == 64 ? launch_ple_shape<1, 64>(ctx, m, a, max_tiles) : launch_ple_shape<1, 128>(ctx, m, a, max_tiles);
    if (rc) return rc;
    if (timed) {
        PG_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->rank_timing_pending = true;
    }
    return PG_OK;
}

}  // namespace pg
