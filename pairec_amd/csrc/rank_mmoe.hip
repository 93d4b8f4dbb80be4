// rank_mmoe.hip — PG_MODEL_MMOE: E gated experts and one tower per task, a candidate's whole forward pass in registers.
//
// The reference's rank fixtures are multi-task answers of one PAI-EAS model (probs_ctr / probs_cvr: EasyrecResponse.multiValModule,
// algorithm/eas/easyrec_response.go:35-70, written back as <algo>_<output> by service/rank/rank_service.go:315-319).  The model
// behind such answers is a multi-gate mixture of experts, x = [u | e]:
//     a_k = relu(We_k' x + be_k)      g_t = softmax_k(Wg_t' x + bg_t)      m_t = sum_k g_t[k] a_k
//     score_t = sigmoid(wo_t . relu(Wt_t' m_t + bt_t) + bo_t)
//
// User half once per request: mmoe_user_partial_kernel writes c1[r] = W_user' u + b over the 32 gate rows and the E h_e
// layer-1 rows as fp32 chains; every accumulator of the big product starts from it, so that product is d_item deep.
//
// Work split: one workgroup of 4 waves per tile of up to 128 candidates of one request (the trunk's tile builder), candidates on
// the MFMA column axis as in rank_din.hip — wave w the items 32 w .. 32 w + 31, lane (j, hk) item j.  A lane reads its item's row
// from the table straight into B-operand registers (lane (j, hk) holds e[16 ks + 8 hk + 0..7] of every k-group ks), where it stays
// for the gate block and all of layer 1.
//
// Row order chosen at pack time (rank_model.hpp: pack_mmoe, mmoe_slot).  In a v_mfma_f32_32x32x16_bf16 accumulator lane (j, hk)
// holds rows (r & 3) + 8 (r >> 2) + 4 hk, r = 0..15, of item j.  The host places the weights' rows so that
//   * the gate block's slot G = 16 hk + r is logit (task G / E, expert G % E): a lane half holds whole tasks, the softmax
//     (max-subtracted, expf) runs over the lane's own registers and ONE exchange between the halves hands each lane all T E gates;
//   * layer 1 runs in steps of 16 hidden units x E experts = E / 2 blocks, slot q = 16 b + r of a step being (expert q % E, hidden
//     unit 16 s + 8 hk + q / E): after a step a lane holds all experts of hidden units 16 s + 8 hk + 0..7 — relu and the mix
//     m_t[j] = sum_k g_t[k] a_k[j] run over its own registers, and the 8 mixed values are exactly the 8 consecutive k it must
//     supply as the tower product's B operand for that 16-deep slice.
// No activation is written to LDS, and neither the E h_e activations nor the T h_e mixed values are ever live at once: after each
// step the lane mixes, converts (or splits) to bf16 and issues the tower MFMAs of the slice into T h_t / 32 accumulator blocks
// (tasks are padded to TP = 2 or 4 with zero weights; a padded task is computed and not stored).
//
// LDS holds weights only, one record per step packed contiguously on the host in fragment order (1 KiB per fragment, a lane's
// 16 B at 16 lane: conflict-free): the step's E / 2 x d_item / 16 layer-1 fragments, then the towers' TP h_t / 32 fragments of the
// slice.  The gate record (d_item / 16 fragments) sits in front.  Records are double-buffered — the next step's record is
// requested from global memory before this step's MFMAs and written to the other buffer after them, one barrier per step — except
// where two buffers would pass 128 KB (E = 8, d_item = 128 in BF16X3: 72 or 80 KB per record), which runs single-buffered with two
// barriers per step.  Worst double-buffered case, (4, 128), T = 4, h_t = 64, d_item = 128, BF16X3: 24 + 2 x 48 = 120 KB.
//
// Two forms of one body (NP products per term).  BF16 (NP 1): the candidate row, every weight and each m_t rounded once (RNE).
// BF16X3 (NP 3): exactly those operands split into hi + lo (split_bf16x2; the weights on the host), lo.hi + hi.lo + hi.hi.
// c1, the accumulation, the biases, relu, the softmax, the mix, the head dot and the sigmoid are fp32 in both.  The gate block of
// the BF16X3 form alone splits its operands THREE ways (hi + mid + lo = the fp32 value exactly) and takes the six products down to
// 2^-16: a logit is an exponent, and the 2^-18 a two-way split leaves of a +-80 logit showed as 4.7e-7 of a score.
//
// Epilogue per lane: the tower accumulators start at bt, so relu and the wo_t dot over the lane's 16 rows per block, one exchange
// between the halves, bo_t, sigmoid, one coalesced store per task plane.
#include "rank_mlp.hpp"

namespace pg {

struct MmoeArgs {
    const uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles;
    const float* tab;
    uint32_t tab_rows;
    const uint32_t* cand_rows;
    const float* c1;            // [n_req][nc]
    uint32_t nc;                // 32 + E h_e
    uint32_t steps;             // h_e / 16
    const char* rec;            // the gate record, then one record per step
    const float *bt, *wo, *bo;  // [TP][h_t], [TP][h_t], [TP]
    uint32_t n_task;
    float* out;
    size_t out_stride;
};

// c1[r][c] = chain(bu[c]; u[r][k] * wu[k][c], k ascending): the user is not rounded, wu is stored in the model's operand precision
__global__ void mmoe_user_partial_kernel(const float* __restrict__ user, uint32_t du, const float* __restrict__ wu,
                                         const float* __restrict__ bu, uint32_t nc, float* __restrict__ c1) {
    const uint32_t r = blockIdx.x;
    const uint32_t c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const float* const u = user + (size_t)r * du;
    float acc = bu[c];
    uint32_t k = 0;
    for (; k + 16 <= du; k += 16) {
        float wv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) wv[i] = wu[(size_t)(k + i) * nc + c];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = __fmaf_rn(u[k + i], wv[i], acc);
    }
    for (; k < du; ++k) acc = __fmaf_rn(u[k], wu[(size_t)k * nc + c], acc);
    c1[(size_t)r * nc + c] = acc;
}

int mmoe_user_partial_launch(pg_ctx* ctx, const float* d_user, uint32_t n_req, uint32_t du, const float* wu, const float* bu, uint32_t nc,
                             float* c1) {
    mmoe_user_partial_kernel<<<dim3(n_req, (nc + 255) / 256), 256, 0, ctx->stream>>>(d_user, du, wu, bu, nc, c1);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

constexpr int mmoe_nbuf(int gate_bytes, int step_bytes) { return gate_bytes + 2 * step_bytes <= 128 * 1024 ? 2 : 1; }

template <int NP, int D, int E, int TP, int HT>
__global__ __launch_bounds__(256) void mmoe_kernel(MmoeArgs a) {
    constexpr int KS = D / 16;                  // k-groups of the d_item-deep product
    constexpr int EB = E / 2;                   // layer-1 blocks per step
    constexpr int HB = HT / 32, NTB = TP * HB;  // tower blocks
    constexpr int FRAG = (NP == 3 ? 2 : 1) * 1024;
    constexpr int GFRAG = (NP == 3 ? 3 : 1) * 1024;
    constexpr int GBYTES = KS * GFRAG, L1BYTES = EB * KS * FRAG, SBYTES = L1BYTES + NTB * FRAG;
    constexpr int NBUF = mmoe_nbuf(GBYTES, SBYTES);
    constexpr int NLD = (SBYTES / 16 + 255) / 256;      // 16-B loads per thread and record
    constexpr int NG = TP * E;                  // gates a lane needs
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    static_assert((E == 2 || E == 4 || E == 8) && (TP == 2 || TP == 4) && (HT == 32 || HT == 64) && (D == 64 || D == 128), "shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const GT = smem;                      // the gate record
    char* const BUF = smem + GBYTES;            // NBUF step records

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
    const char* const steps_rec = a.rec + GBYTES;

    // ---- the gate record and step 0's record into LDS ----------------------------------------------------------------------
    for (int i = tid; i < GBYTES / 16; i += 256) reinterpret_cast<u32x4*>(GT)[i] = reinterpret_cast<const u32x4*>(a.rec)[i];
    for (int i = tid; i < SBYTES / 16; i += 256) reinterpret_cast<u32x4*>(BUF)[i] = reinterpret_cast<const u32x4*>(steps_rec)[i];

    // ---- this lane's item: its row as B-operand registers ------------------------------------------------------------------
    const uint32_t r_item = wave * 32 + j;
    const bool live = r_item < cnt;
    uint32_t erow = a.cand_rows[item0 + (live ? r_item : cnt - 1)];
    erow = erow < a.tab_rows ? erow : a.tab_rows - 1;
    const float4* const ep = reinterpret_cast<const float4*>(a.tab + (size_t)erow * D);
    bf16x8 eh[KS], el[NP == 3 ? KS : 1], e3[NP == 3 ? KS : 1];     // (e3: the third part, for the gate block only)
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

    // ---- the gates: one block, softmax over the lane's own registers, one exchange between the halves -----------------------
    float g[NG];
    f32x16 at[NTB];
    if (active) {
        f32x16 ga = mmoe_rows16(c1r);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if constexpr (NP == 3) {            // (w3 e1 + w1 e3 + w2 e2) + (w2 e1 + w1 e2) + w1 e1
                const bf16x8 w3 = *reinterpret_cast<const bf16x8*>(GT + ks * GFRAG + 2048 + lane * 16);
                const bf16x8 w2 = *reinterpret_cast<const bf16x8*>(GT + ks * GFRAG + 1024 + lane * 16);
                const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(GT + ks * GFRAG + lane * 16);
                ga = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3, eh[ks], ga, 0, 0, 0);
                ga = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, e3[ks], ga, 0, 0, 0);
                ga = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, el[ks], ga, 0, 0, 0);
            }
            ga = mmoe_mac<NP>(GT + ks * GFRAG, lane, eh[ks], el[NP == 3 ? ks : 0], ga);
        }
#pragma unroll
        for (int tl = 0; tl < 16 / E; ++tl) {
            float mx = ga[tl * E];
#pragma unroll
            for (int k = 1; k < E; ++k) mx = fmaxf(mx, ga[tl * E + k]);
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                ga[tl * E + k] = expf(ga[tl * E + k] - mx);
                sum = sum + ga[tl * E + k];
            }
#pragma unroll
            for (int k = 0; k < E; ++k) ga[tl * E + k] = ga[tl * E + k] / sum;
        }
        float other[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) other[r] = r < NG ? __shfl_xor(ga[r], 32) : 0.f;
#pragma unroll
        for (int G = 0; G < NG; ++G) g[G] = (G >> 4) == hk ? ga[G & 15] : other[G & 15];
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb) at[tb] = mmoe_rows16(a.bt + tb * 32 + 4 * hk);
    }

    // ---- layer 1 in steps of 16 hidden units x E experts; each step's mix feeds the towers' 16-deep slice -------------------
    for (uint32_t s = 0; s < a.steps; ++s) {
        const char* const cur = BUF + (NBUF == 2 ? (s & 1) * SBYTES : 0);
        const bool more = s + 1 < a.steps;
        const u32x4* const next = reinterpret_cast<const u32x4*>(steps_rec + (size_t)(s + 1) * SBYTES);
        u32x4 pre[NLD];
        if (NBUF == 2 && more) {
#pragma unroll
            for (int c = 0; c < NLD; ++c)
                if (tid + 256 * c < SBYTES / 16) pre[c] = next[tid + 256 * c];
        }
        if (active) {
            f32x16 acc[EB];
#pragma unroll
            for (int b = 0; b < EB; ++b) acc[b] = mmoe_rows16(c1r + 32 + (s * EB + b) * 32);
#pragma unroll
            for (int b = 0; b < EB; ++b) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc[b] = mmoe_mac<NP>(cur + (b * KS + ks) * FRAG, lane, eh[ks], el[NP == 3 ? ks : 0], acc[b]);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[b][r] = fmaxf(acc[b][r], 0.f);
            }
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                float mv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float v = 0.f;
#pragma unroll
                    for (int k = 0; k < E; ++k) v = __fmaf_rn(g[t * E + k], acc[(u * E + k) >> 4][(u * E + k) & 15], v);
                    mv[u] = v;
                }
                bf16x8 mh, ml;
                mmoe_operand<NP>(mv, mh, ml);
#pragma unroll
                for (int hb = 0; hb < HB; ++hb) at[t * HB + hb] = mmoe_mac<NP>(cur + L1BYTES + (t * HB + hb) * FRAG, lane, mh, ml, at[t * HB + hb]);
            }
        }
        if (NBUF == 2) {
            if (more) {
                u32x4* const dst = reinterpret_cast<u32x4*>(BUF + ((s + 1) & 1) * SBYTES);      // last read in step s - 1
#pragma unroll
                for (int c = 0; c < NLD; ++c)
                    if (tid + 256 * c < SBYTES / 16) dst[tid + 256 * c] = pre[c];
            }
            __syncthreads();
        } else if (more) {
            __syncthreads();                    // every wave has read the record
            for (int i = tid; i < SBYTES / 16; i += 256) reinterpret_cast<u32x4*>(BUF)[i] = next[i];
            __syncthreads();
        }
    }
    if (!active) return;

    // ---- the towers' heads: relu, the wo dot over the lane's rows and its partner's, bo, sigmoid ----------------------------
#pragma unroll
    for (int t = 0; t < TP; ++t) {
        float v = 0.f;
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            const f32x16 w = mmoe_rows16(a.wo + (t * HB + hb) * 32 + 4 * hk);
#pragma unroll
            for (int r = 0; r < 16; ++r) v = __fmaf_rn(w[r], fmaxf(at[t * HB + hb][r], 0.f), v);
        }
        v = v + __shfl_xor(v, 32);
        const float z = v + a.bo[t];
        if ((uint32_t)t < a.n_task && live && hk == 0) a.out[(size_t)t * a.out_stride + item0 + r_item] = 1.0f / (1.0f + expf(-z));
    }
}

template <int NP, int D, int E, int TP, int HT>
static int launch_mmoe(pg_ctx* ctx, const MmoeArgs& a, uint32_t grid) {
    constexpr int gate = (int)mmoe_gate_bytes(D, NP == 3 ? 2 : 1), step = (int)mmoe_step_bytes(D, E, TP, HT, NP == 3 ? 2 : 1);
    constexpr size_t lds = gate + (size_t)mmoe_nbuf(gate, step) * step;
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)mmoe_kernel<NP, D, E, TP, HT>, lds))) return rc;
    mmoe_kernel<NP, D, E, TP, HT><<<grid, 256, lds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
template <int NP, int D, int E>
static int launch_mmoe_towers(pg_ctx* ctx, const pg_model* m, const MmoeArgs& a, uint32_t grid) {
    if (m->mm_tp == 2) return m->h_t == 32 ? launch_mmoe<NP, D, E, 2, 32>(ctx, a, grid) : launch_mmoe<NP, D, E, 2, 64>(ctx, a, grid);
    return m->h_t == 32 ? launch_mmoe<NP, D, E, 4, 32>(ctx, a, grid) : launch_mmoe<NP, D, E, 4, 64>(ctx, a, grid);
}
template <int NP>
static int launch_mmoe_shape(pg_ctx* ctx, const pg_model* m, const MmoeArgs& a, uint32_t grid) {
#define X(NE)                                                                                       \
    if (m->n_expert == NE)                                                                          \
        return m->d_item == 64 ? launch_mmoe_towers<NP, 64, NE>(ctx, m, a, grid) : launch_mmoe_towers<NP, 128, NE>(ctx, m, a, grid);
    X(2) X(4) X(8)
#undef X
    set_error("rank: MMoE with %u experts has no kernel", m->n_expert);
    return PG_ERR_UNSUPPORTED;
}

int rank_mmoe_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user, const uint32_t* d_cand,
                         const uint32_t* d_off, uint32_t n_req, uint32_t n_items, float* d_out) {
    if (n_items == 0 || n_req == 0) return PG_OK;
    const uint32_t max_tiles = n_items / kBM + n_req, nc = 32 + m->n_expert * m->h_e;
    float* c1;
    uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles, *req_tile0;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotMmoe, [&](Carve& c) {
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
    MmoeArgs a{};
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
    a.rec = (const char*)m->mm_rec;
    a.bt = m->mm_bt;
    a.wo = m->mm_wo;
    a.bo = m->mm_bo;
    a.n_task = m->n_out;
    a.out = d_out;
    a.out_stride = n_items;
    rc = m->prec == 2 ? launch_mmoe_shape<3>(ctx, m, a, max_tiles) : launch_mmoe_shape<1>(ctx, m, a, max_tiles);
    if (rc) return rc;
    if (timed) {
        PG_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->rank_timing_pending = true;
    }
    return PG_OK;
}

}  // namespace pg
