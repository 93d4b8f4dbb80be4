// rank_dcn.hip — PG_MODEL_DCN: stacked DCN-v2 cross layers and a DNN3 head, a candidate's whole forward pass in registers.
//
// The reference ships no DCN arithmetic: its rank models are remote (algorithm/eas: EasModel.Run sends the request to a PAI-EAS
// EasyRec model and reads scores back).  DCN-v2 is one of that zoo's stock backbones, x_0 = [u | e]:
//     x_{l+1} = x_0 * (Wc_l' x_l + bc_l) + x_l      l = 0 .. L-1  (* element-wise)
//     score_o = sigmoid(w3[:, o] . relu(W2' relu(W1' x_L + b1) + b2) + b3[o])
//
// Feature order (rank_model.hpp: pack_dcn).  The kernel keeps x in the order item columns, user columns, zero padding up to
// DP = 128, 192 or 256, so that the item row a lane reads is at once layer 0's matrix operand and the item part of x_0.
//
// User half once per request: dcn_user_partial_kernel writes c0[r] = Wc_0[user rows]' u + bc_0 as fp32 chains and, behind it,
// x_0's user and padding columns; layer 0's product is d_item deep and its accumulators start at c0.  From x_1 on the user
// coordinates differ per candidate, so nothing later is hoisted.
//
// Work split: one workgroup of 4 waves per tile of up to 128 candidates of one request (the trunk's tile builder), candidates on
// the MFMA column axis — wave w the items 32 w .. 32 w + 31, lane (j, hk) item j.  A 32-feature block of any vector of a
// candidate is 16 registers of each of its two lanes, register r = feature 16 (r >> 3) + 8 hk + (r & 7): registers 0..7 and
// 8..15 are the 8 consecutive k a lane supplies as the B operand of a v_mfma_f32_32x32x16_bf16 for the block's two 16-deep
// slices.  The loader permutes every matrix's OUTPUT columns so that an accumulator block comes out in exactly this order
// (dcn_row): the accumulators of one product are the operand registers of the next with no LDS round trip, converted (or split)
// to bf16 one slice at a time as they are consumed.  Every product — a cross layer, W1, W2 — is therefore the same step: one
// input block (two slices) against all NBO output blocks, 2 NBO independent accumulator chains.
//
// Live state per lane at DP = 256, d_item = 128: 128 registers of x_l (no block of it may be overwritten before the layer's last
// step has read it), 128 accumulators, 64 of the item row in fp32 (x_0's item part; x_0's user part is per request and is read
// from c0's row when a layer ends), up to 32 of the record in flight: one wave per SIMD, the accumulators in the AGPR half.
// The tile stays at 128 candidates because that state fills the register file: a second 32-candidate block per wave has no room.
//
// LDS holds weights only.  A record (host-packed, fragment order: 1 KiB per fragment, a lane's 16 B at 16 lane, conflict-free)
// is one input block of one matrix against all its output blocks: 2 NBO fragments, 8 to 32 KB.  Records are consumed in one
// sequence — layer 0's d_item / 32, DP / 32 per further layer (a run-time loop: one body serves every n_cross), DP / 32 of W1,
// h1 / 32 of W2 — and EVERY instantiation double-buffers them (2 x 32 KB at most): the next record is requested from global
// memory before a step's MFMAs and written to the other buffer after them, one barrier per step.
//
// Two forms of one body (NP products per term).  BF16 (NP 1): the candidate row as layer 0's operand, every weight matrix, and
// x_l (l >= 1), x_L and h1 as operands are rounded once (RNE).  BF16X3 (NP 3): exactly those split into hi + lo (the weights on
// the host), lo.hi + hi.lo + hi.hi.  u, c0, the accumulation, the biases, x_0 and x_l in the element-wise product and the
// residual, relu, the head dot and the sigmoid are fp32 in both.
#include "rank_mlp.hpp"

namespace pg {

struct DcnArgs {
    const uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles;
    const float* tab;
    uint32_t tab_rows;
    const uint32_t* cand_rows;
    const float* c0;            // [n_req][2 DP]: c0, then x_0 (its item columns unused)
    const float* bc;            // [n_cross][DP]
    uint32_t n_cross;
    const char* rec;
    const float *b1, *b2, *w3, *b3;     // [h1], [128], [n_out][128], [n_out]
    uint32_t n_out;
    float* out;
    size_t out_stride;
};

// c0[r][g] = chain(bc_0[g]; u[r][k] * wu[k][g], k ascending): the user is not rounded, wu is stored in the operand precision;
// x_0[r][g] = u[r][g - d_item] on the user columns, 0 elsewhere
__global__ void dcn_user_partial_kernel(const float* __restrict__ user, uint32_t du, uint32_t di, const float* __restrict__ wu,
                                        const float* __restrict__ bc0, uint32_t dp, float* __restrict__ c0) {
    const uint32_t r = blockIdx.x, g = threadIdx.x;
    const float* const u = user + (size_t)r * du;
    float acc = bc0[g];
    for (uint32_t k = 0; k < du; ++k) acc = __fmaf_rn(u[k], wu[(size_t)k * dp + g], acc);
    c0[(size_t)r * 2 * dp + g] = acc;
    c0[(size_t)r * 2 * dp + dp + g] = g >= di && g < di + du ? u[g - di] : 0.0f;
}

// acc += A' B with A the fragment at `frag` (split: its lo fragment 1 KiB on) and B = bh (+ bl)
template <int NP>
__device__ __forceinline__ f32x16 dcn_mac(const char* frag, int lane, bf16x8 bh, bf16x8 bl, f32x16 acc) {
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(frag + lane * 16);
    if constexpr (NP == 3) {
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(frag + 1024 + lane * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// one input block `in` (two k-slices) against the NBO output blocks of the record at `cur`
template <int NP, int NBO>
__device__ __forceinline__ void dcn_step(const char* cur, int lane, const f32x16& in, f32x16 (&acc)[NBO]) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int FRAG = (NP == 3 ? 2 : 1) * 1024;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        uint32_t ph[4], pl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v0 = in[8 * s + 2 * i], v1 = in[8 * s + 2 * i + 1];
            if constexpr (NP == 3) {
                split_bf16x2(v0, v1, ph[i], pl[i]);
            } else {
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
                ph[i] = pl[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v0, v1}, bf16x2));   // v_cvt_pk_bf16_f32 (RNE); lo is not read
            }
        }
        const bf16x8 bh = __builtin_bit_cast(bf16x8, (u32x4){ph[0], ph[1], ph[2], ph[3]});
        const bf16x8 bl = __builtin_bit_cast(bf16x8, (u32x4){pl[0], pl[1], pl[2], pl[3]});
#pragma unroll
        for (int b = 0; b < NBO; ++b) acc[b] = dcn_mac<NP>(cur + (s * NBO + b) * FRAG, lane, bh, bl, acc[b]);
    }
}

// the lane's 16 registers of a 32-feature block of an fp32 vector in feature order (p = block + 8 hk): p[0..7] and p[16..23]
__device__ __forceinline__ f32x16 dcn_block16(const float* p) {
    f32x16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 c = *reinterpret_cast<const float4*>(p + 4 * (q & 1) + 16 * (q >> 1));
        v[4 * q + 0] = c.x; v[4 * q + 1] = c.y; v[4 * q + 2] = c.z; v[4 * q + 3] = c.w;
    }
    return v;
}

constexpr int dcn_max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
// the largest record of an instantiation: one LDS buffer (there are two)
constexpr int dcn_buf_bytes(int dp, int h1, int np) { return dcn_max3(dp, h1, 128) / 32 * 2 * (np == 3 ? 2 : 1) * 1024; }

template <int NP, int DP, int DI, int H1>
__global__ __launch_bounds__(256) void dcn_kernel(DcnArgs a) {
    constexpr int NB = DP / 32, IB = DI / 32, NB1 = H1 / 32, NB2 = 4;
    constexpr int FRAG = (NP == 3 ? 2 : 1) * 1024;
    constexpr uint32_t CB = 2 * NB * FRAG, W1B = 2 * NB1 * FRAG, W2B = 2 * NB2 * FRAG;      // record bytes per phase
    constexpr int RB = dcn_buf_bytes(DP, H1, NP);
    constexpr int NLD = RB / 16 / 256;          // 16-B loads per thread and record
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    static_assert((DP == 128 || DP == 192 || DP == 256) && (DI == 64 || DI == 128) && DI < DP && (H1 == 128 || H1 == 256), "shape");
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

    // ---- the record stream: record i lives in buffer i & 1; a step requests record i + 1 before its MFMAs (fetch) and writes
    // it to the other buffer, last read in step i - 1, after them (commit: one barrier) -------------------------------------------
    u32x4 pre[NLD];
    const char* next = a.rec;
    uint32_t nrec = 0;
    auto fetch = [&](uint32_t nbytes) {
#pragma unroll
        for (int c = 0; c < NLD; ++c)
            if ((uint32_t)(tid + 256 * c) * 16 < nbytes) pre[c] = reinterpret_cast<const u32x4*>(next)[tid + 256 * c];
    };
    auto commit = [&](uint32_t nbytes) {
        u32x4* const dst = reinterpret_cast<u32x4*>(smem + (nrec & 1) * RB);
#pragma unroll
        for (int c = 0; c < NLD; ++c)
            if ((uint32_t)(tid + 256 * c) * 16 < nbytes) dst[tid + 256 * c] = pre[c];
        next += nbytes;
        ++nrec;
        __syncthreads();
    };
    fetch(CB);

    // ---- this lane's item: its half of the row in fp32, block by block ------------------------------------------------------------
    const uint32_t r_item = wave * 32 + j;
    const bool live = r_item < cnt;
    uint32_t erow = a.cand_rows[item0 + (live ? r_item : cnt - 1)];
    erow = erow < a.tab_rows ? erow : a.tab_rows - 1;
    f32x16 eb[IB];
#pragma unroll
    for (int b = 0; b < IB; ++b) eb[b] = dcn_block16(a.tab + (size_t)erow * DI + 32 * b + 8 * hk);
    const float* const c0r = a.c0 + (size_t)req * 2 * DP + 8 * hk;
    const float* const x0r = c0r + DP;
    commit(CB);

    // ---- layer 0: d_item deep from c0; x_1 = x_0 * t + x_0 ---------------------------------------------------------------------
    f32x16 x[NB];
    {
        f32x16 acc[NB];
        if (active) {
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = dcn_block16(c0r + 32 * b);
        }
#pragma unroll
        for (int kb = 0; kb < IB; ++kb) {
            const char* const cur = smem + ((nrec - 1) & 1) * RB;
            const uint32_t nn = kb + 1 < IB || a.n_cross > 1 ? CB : W1B;
            fetch(nn);
            if (active) dcn_step<NP, NB>(cur, lane, eb[kb], acc);
            commit(nn);
        }
        if (active) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                f32x16 x0;
                if (b < IB) x0 = eb[b < IB ? b : 0];
                else x0 = dcn_block16(x0r + 32 * b);
                x[b] = x0 * acc[b] + x0;
            }
        }
    }

    // ---- layers 1 .. L-1: DP deep from bc_l; x_{l+1} = x_0 * t + x_l, written only after the layer's last step ----------------------
    for (uint32_t l = 1; l < a.n_cross; ++l) {
        f32x16 acc[NB];
        if (active) {
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = dcn_block16(a.bc + (size_t)l * DP + 32 * b + 8 * hk);
        }
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
            const char* const cur = smem + ((nrec - 1) & 1) * RB;
            const uint32_t nn = kb + 1 < NB || l + 1 < a.n_cross ? CB : W1B;
            fetch(nn);
            if (active) dcn_step<NP, NB>(cur, lane, x[kb], acc);
            commit(nn);
        }
        if (active) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                f32x16 x0;
                if (b < IB) x0 = eb[b < IB ? b : 0];
                else x0 = dcn_block16(x0r + 32 * b);
                x[b] = x0 * acc[b] + x[b];
            }
        }
    }

    // ---- W1: h1 = relu(W1' x_L + b1) -----------------------------------------------------------------------------------------
    f32x16 h[NB1];
    if (active) {
#pragma unroll
        for (int b = 0; b < NB1; ++b) h[b] = dcn_block16(a.b1 + 32 * b + 8 * hk);
    }
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        const char* const cur = smem + ((nrec - 1) & 1) * RB;
        const uint32_t nn = kb + 1 < NB ? W1B : W2B;
        fetch(nn);
        if (active) dcn_step<NP, NB1>(cur, lane, x[kb], h);
        commit(nn);
    }

    // ---- W2: h2 = relu(W2' h1 + b2) ------------------------------------------------------------------------------------------
    f32x16 g2[NB2];
    if (active) {
#pragma unroll
        for (int b = 0; b < NB1; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) h[b][r] = fmaxf(h[b][r], 0.f);
#pragma unroll
        for (int b = 0; b < NB2; ++b) g2[b] = dcn_block16(a.b2 + 32 * b + 8 * hk);
    }
#pragma unroll
    for (int kb = 0; kb < NB1; ++kb) {
        const char* const cur = smem + ((nrec - 1) & 1) * RB;
        const uint32_t nn = kb + 1 < NB1 ? W2B : 0;
        fetch(nn);
        if (active) dcn_step<NP, NB2>(cur, lane, h[kb], g2);
        commit(nn);
    }
    if (!active) return;

    // ---- the heads: relu, the w3 dot over the lane's registers and its partner's, b3, sigmoid -------------------------------------
    for (uint32_t o = 0; o < a.n_out; ++o) {
        float v = 0.f;
#pragma unroll
        for (int b = 0; b < NB2; ++b) {
            const f32x16 w = dcn_block16(a.w3 + (size_t)o * 128 + 32 * b + 8 * hk);
#pragma unroll
            for (int r = 0; r < 16; ++r) v = __fmaf_rn(w[r], fmaxf(g2[b][r], 0.f), v);
        }
        v = v + __shfl_xor(v, 32);
        const float z = v + a.b3[o];
        if (live && hk == 0) a.out[(size_t)o * a.out_stride + item0 + r_item] = 1.0f / (1.0f + expf(-z));
    }
}

template <int NP, int DP, int DI, int H1>
static int launch_dcn(pg_ctx* ctx, const DcnArgs& a, uint32_t grid) {
    constexpr size_t lds = 2 * (size_t)dcn_buf_bytes(DP, H1, NP);
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)dcn_kernel<NP, DP, DI, H1>, lds))) return rc;
    dcn_kernel<NP, DP, DI, H1><<<grid, 256, lds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
template <int NP>
static int launch_dcn_shape(pg_ctx* ctx, const pg_model* m, const DcnArgs& a, uint32_t grid) {
#define X(P, I)                                                                                     \
    if (m->dc_dp == P && m->d_item == I)                                                            \
        return m->h1 == 128 ? launch_dcn<NP, P, I, 128>(ctx, a, grid) : launch_dcn<NP, P, I, 256>(ctx, a, grid);
    X(128, 64) X(192, 64) X(256, 64) X(192, 128) X(256, 128)
#undef X
    set_error("rank: DCN padded to %u columns with d_item %u has no kernel", m->dc_dp, m->d_item);
    return PG_ERR_UNSUPPORTED;
}

int rank_dcn_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user, const uint32_t* d_cand,
                        const uint32_t* d_off, uint32_t n_req, uint32_t n_items, float* d_out) {
    if (n_items == 0 || n_req == 0) return PG_OK;
    const uint32_t max_tiles = n_items / kBM + n_req, dp = m->dc_dp;
    float* c0;
    uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles, *req_tile0;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotDcn, [&](Carve& c) {
            tile_req = c.take<uint32_t>(max_tiles);
            tile_item0 = c.take<uint32_t>(max_tiles);
            tile_cnt = c.take<uint32_t>(max_tiles);
            n_tiles = c.take<uint32_t>(64);
            req_tile0 = c.take<uint32_t>(n_req);
            c0 = c.take<float>((size_t)n_req * 2 * dp);
        }))) return rc;
    const bool timed = !ctx->timers_off;
    if (timed) PG_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((rc = build_tiles_launch(ctx, d_off, n_req, max_tiles, kBM, tile_req, tile_item0, tile_cnt, n_tiles, req_tile0))) return rc;
    dcn_user_partial_kernel<<<n_req, dp, 0, ctx->stream>>>(d_user, m->d_user, m->d_item, m->dc_wu, m->dc_bc, dp, c0);
    PG_HIP(hipGetLastError());
    DcnArgs a{};
    a.tile_req = tile_req;
    a.tile_item0 = tile_item0;
    a.tile_cnt = tile_cnt;
    a.n_tiles = n_tiles;
    a.tab = t->d;
    a.tab_rows = (uint32_t)t->rows;
    a.cand_rows = d_cand;
    a.c0 = c0;
    a.bc = m->dc_bc;
    a.n_cross = m->n_cross;
    a.rec = (const char*)m->dc_rec;
    a.b1 = m->b1;
    a.b2 = m->b2;
    a.w3 = m->w3;
    a.b3 = m->b3v;
    a.n_out = m->n_out;
    a.out = d_out;
    a.out_stride = n_items;
    rc = m->prec == 2 ? launch_dcn_shape<3>(ctx, m, a, max_tiles) : launch_dcn_shape<1>(ctx, m, a, max_tiles);
    if (rc) return rc;
    if (timed) {
        PG_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->rank_timing_pending = true;
    }
    return PG_OK;
}

}  // namespace pg
