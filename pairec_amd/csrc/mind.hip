// mind.hip — PG_MODEL_MIND: a user's behaviour sequence routed into K interest capsules (B2I dynamic routing), each capsule
// through a two-layer head with the user vector; pg_mind_interests[_dev], and pg_mind_recall[_dev]: every interest one query of
// the exact inner-product recall (the reference's rule for a model that answers several embeddings joined by "|",
// service/recall/online_hologres_vector_recall.go:186-223).  The arithmetic is include/pairec_gpu.h's; the summation orders are
// DESIGN.md §5 item 15.
//
// mind_kernel, one workgroup of 4 waves per request; the routing loop never leaves the chip.  Every product is a
// v_mfma_f32_16x16x4_f32: lane (i, g) = (lane & 15, lane >> 4) supplies A[i][g] and B[g][i], and holds D[4 g + r][i], r = 0..3.
//
//   prologue.  The entries past the table are dropped by ballot rank (n valid rows, in order).  U^ = seq . S, position tiles of
//              16 dealt to the waves: a lane's A operand is read straight from its position's table row (four 16-byte reads,
//              depth 16 s + 4 g + e for step (s, e)), S is the B operand, all of it in 64 registers per lane, read once from L2.
//              A position >= n supplies zeros, so the last tile's tail rows of U^ are zero.
//   iteration. softmax over k: thread = position, the K logits in registers for the whole loop (b0 at first, then += the
//              delta the previous iteration left in LDS); the weights go to LDS, zero for a position >= n.
//              Z = W . U^: capsules on the row side (lane i >= K supplies zero), wave w the columns 16 w .. 16 w + 15, depth =
//              the positions, step t of tile T the positions 16 T + 4 g + t (one 16-byte read of W per tile and lane).
//              squash: |z_k|^2 over a wave's 16 columns by an xor butterfly, over the four waves through LDS; V (16 x 64,
//              rows >= K zero) to LDS.
//              dB = U^ . V^T: position tiles dealt to the waves, capsules on the column side, depth 64 as in the prologue; V's
//              operand registers are read once per iteration.  The delta goes where the weights were.
//   head.      Wu'u + Wc'v_k for the K capsules at once, thread = hidden unit (coalesced weight rows); W2'h_k, thread =
//              (output column, capsule group); the optional normalisation, wave = capsule.
//
// LDS (78 480 bytes: two workgroups per CU of 160 KB):
//     U^   [256][64] fp32, 65 536 B, NOT padded: the 16-byte group c4 of row p lives at group c4 ^ (p & 15).  The prologue's
//          stores (lane (i, g) -> row 4 g + r, column 16 cb + i), the Z product's loads (row 4 g + t, column 16 w + i) and the
//          delta product's 16-byte loads (row i, group 4 s + g) are then all conflict-free; a pitch of 68 serves only two of
//          the three and would put the workgroup past 80 KB.
//     WD   [8][260]: the softmax weights, then the logits' delta (same thread, same address: no hazard)
//     V    [16][68]; the compacted rows [256] live here during the prologue
//     PART [4][16] partial |z|^2, and the four ballot counts
//     after the loop U^ is dead: the user vector [1024], H [8][256] and the interests [8][128] take its place.
#include "rank_mlp.hpp"

namespace pg {

constexpr int kMindLP = (int)kMindSeq + 4;     // pitch of WD's rows: 16-byte aligned, row k starts 4 k banks on
constexpr int kMindVP = (int)kMindD + 4;       // pitch of V's rows
constexpr int kMindLds = ((int)kMindSeq * (int)kMindD + (int)kMindMaxK * kMindLP + 16 * kMindVP + 64 + 4) * 4;
static_assert(kMindLds <= 80 * 1024, "two workgroups per CU");
static_assert(1024 + kMindMaxK * 256 + kMindMaxK * 128 <= kMindSeq * kMindD, "the head's buffers fit where U^ was");

struct MindArgs {
    const float* tab;
    uint32_t tab_rows;
    const uint32_t *seq_rows, *seq_off;
    const float* user;
    const float *S, *b0, *Wc, *Wu, *b1, *W2, *b2;
    float* out;                                 // [n_req][K][d_out]
    uint32_t d_user, d_out, K, n_iter, h1, normalize;
};

// U^[row][col .. col + 3] (col a multiple of 4 for a 16-byte access)
__device__ __forceinline__ int mind_u(int row, int col) { return row * (int)kMindD + ((((col >> 2) ^ row) & 15) << 2) + (col & 3); }

#define MIND_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)

__global__ __launch_bounds__(256) void mind_kernel(MindArgs a) {
    constexpr int D = kMindD, MAXK = kMindMaxK;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const U = smem;
    float* const WD = U + kMindSeq * D;
    float* const V = WD + MAXK * kMindLP;
    float* const PART = V + 16 * kMindVP;
    uint32_t* const wcnt = reinterpret_cast<uint32_t*>(PART + 64);
    uint32_t* const rows = reinterpret_cast<uint32_t*>(V);

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int K = (int)a.K;
    const uint32_t s0 = a.seq_off[r], s1 = a.seq_off[r + 1];
    const int L = s1 > s0 ? (s1 - s0 < kMindSeq ? (int)(s1 - s0) : (int)kMindSeq) : 0;

    // ---- the valid entries, in order: rank by ballot within a wave, by the waves' counts across them -----------------------------
    uint32_t row = 0;
    bool ok = false;
    if (tid < L) {
        row = a.seq_rows[s0 + tid];
        ok = row < a.tab_rows;
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += (int)wcnt[w];
    if (ok) rows[before + __popcll(bal & ((1ull << lane) - 1))] = row;
    const int n = (int)(wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
    const int nt = (n + 15) >> 4;
    __syncthreads();

    // ---- U^ = seq . S -------------------------------------------------------------------------------------------------------------
    {
        float sreg[4][4][4];                    // S[16 s + 4 g + e][16 cb + i]
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) sreg[s][e][cb] = a.S[(16 * s + 4 * g + e) * D + 16 * cb + i];
        for (int T = wave; T < nt; T += 4) {
            const int pos = 16 * T + i;
            f32x4 av[4] = {};
            if (pos < n) {
                const float* const rp = a.tab + (size_t)rows[pos] * D + 4 * g;
#pragma unroll
                for (int s = 0; s < 4; ++s) av[s] = *reinterpret_cast<const f32x4*>(rp + 16 * s);
            }
            f32x4 acc[4] = {};
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) acc[cb] = MIND_MFMA(av[s][e], sreg[s][e][cb], acc[cb]);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) U[mind_u(16 * T + 4 * g + rr, 16 * cb + i)] = acc[cb][rr];
        }
    }
    __syncthreads();                            // (the rows are dead from here: V may be written)

    // ---- the routing loop -----------------------------------------------------------------------------------------------------------
    float bl[MAXK];                             // position tid's logits
#pragma unroll
    for (int k = 0; k < MAXK; ++k) bl[k] = k < K ? a.b0[k * (int)kMindSeq + tid] : 0.f;
    for (uint32_t it = 1;; ++it) {
        // softmax over the capsules
        if (it > 1) {
#pragma unroll
            for (int k = 0; k < MAXK; ++k)
                if (k < K) bl[k] += WD[k * kMindLP + tid];
        }
        float mx = bl[0];
#pragma unroll
        for (int k = 1; k < MAXK; ++k)
            if (k < K) mx = fmaxf(mx, bl[k]);
        float ex[MAXK], sum = 0.f;
#pragma unroll
        for (int k = 0; k < MAXK; ++k) {
            ex[k] = k < K ? expf(bl[k] - mx) : 0.f;
            sum += ex[k];
        }
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) WD[k * kMindLP + tid] = tid < n ? ex[k] / sum : 0.f;
        __syncthreads();

        // Z = W . U^
        f32x4 z = {};
        for (int T = 0; T < nt; ++T) {
            f32x4 wa = {};
            if (i < K) wa = *reinterpret_cast<const f32x4*>(WD + i * kMindLP + 16 * T + 4 * g);
#pragma unroll
            for (int t = 0; t < 4; ++t) z = MIND_MFMA(wa[t], U[mind_u(16 * T + 4 * g + t, 16 * wave + i)], z);
        }

        // squash: z[rr] is Z[capsule 4 g + rr][column 16 wave + i]
        f32x4 q = z * z;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) q[rr] += __shfl_xor(q[rr], m);
        if (i == 0)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) PART[wave * 16 + 4 * g + rr] = q[rr];
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int c = 4 * g + rr;
            const float qq = ((PART[c] + PART[16 + c]) + PART[32 + c]) + PART[48 + c];
            V[c * kMindVP + 16 * wave + i] = z[rr] * (qq / ((1.f + qq) * sqrtf(qq + 1e-9f)));
        }
        __syncthreads();
        if (it >= a.n_iter) break;

        // dB = U^ . V^T into WD (every wave is past its reads of the weights)
        f32x4 vb[4];                            // V[capsule i][16 s + 4 g + e]
#pragma unroll
        for (int s = 0; s < 4; ++s) vb[s] = *reinterpret_cast<const f32x4*>(V + i * kMindVP + 16 * s + 4 * g);
        for (int T = wave; T < nt; T += 4) {
            f32x4 acc = {};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const f32x4 ua = *reinterpret_cast<const f32x4*>(U + mind_u(16 * T + i, 16 * s + 4 * g));
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = MIND_MFMA(ua[e], vb[s][e], acc);
            }
            if (i < K) *reinterpret_cast<f32x4*>(WD + i * kMindLP + 16 * T + 4 * g) = acc;     // positions 16 T + 4 g + 0..3 of capsule i
        }
        __syncthreads();
    }

    // ---- the head (U^ is dead; V holds the capsules, rows >= K zero) ------------------------------------------------------------------
    float* const UV = U;
    float* const H = U + 1024;
    float* const OUT = H + MAXK * 256;
    const int h1 = (int)a.h1, dout = (int)a.d_out;
    for (uint32_t d = tid; d < a.d_user; d += 256) UV[d] = a.user[(size_t)r * a.d_user + d];
    __syncthreads();
    if (tid < h1) {
        float hu = 0.f;
        for (uint32_t d = 0; d < a.d_user; ++d) hu = fmaf(a.Wu[(size_t)d * h1 + tid], UV[d], hu);
        float hc[MAXK] = {};
        for (int d = 0; d < D; ++d) {
            const float w = a.Wc[d * h1 + tid];
#pragma unroll
            for (int k = 0; k < MAXK; ++k) hc[k] = fmaf(w, V[k * kMindVP + d], hc[k]);
        }
        const float b = a.b1[tid];
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) H[k * 256 + tid] = fmaxf((hc[k] + hu) + b, 0.f);
    }
    __syncthreads();
    {
        // thread = (output column o, capsule group): capsules grp, grp + ng, .. (at most four of them)
        const int o = tid & (dout - 1), grp = tid / dout, ng = 256 / dout;
        float acc[4] = {};
        for (int c = 0; c < h1; ++c) {
            const float w = a.W2[c * dout + o];
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (grp + x * ng < K) acc[x] = fmaf(w, H[(grp + x * ng) * 256 + c], acc[x]);
        }
        const float b = a.b2[o];
#pragma unroll
        for (int x = 0; x < 4; ++x)
            if (grp + x * ng < K) OUT[(grp + x * ng) * 128 + o] = acc[x] + b;
    }
    __syncthreads();
    for (int k = wave; k < K; k += 4) {
        float inv = 1.f;
        if (a.normalize) {
            float ss = 0.f;
            for (int o = lane; o < dout; o += 64) ss = fmaf(OUT[k * 128 + o], OUT[k * 128 + o], ss);
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m);
            inv = sqrtf(ss + 1e-12f);
        }
        for (int o = lane; o < dout; o += 64) a.out[((size_t)r * K + k) * dout + o] = a.normalize ? OUT[k * 128 + o] / inv : OUT[k * 128 + o];
    }
}

// the interests of n_req requests, enqueued: the caller holds ctx->mu and the table's shared lock, and has checked the arguments
static int mind_interests_locked(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user, const uint32_t* d_seq_rows,
                                 const uint32_t* d_seq_off, uint32_t n_req, float* d_out) {
    const MindLayout lay(m->d_user, m->mi_dout, m->n_out, m->h1);
    MindArgs a{};
    a.tab = t->d;
    a.tab_rows = (uint32_t)t->rows;
    a.seq_rows = d_seq_rows;
    a.seq_off = d_seq_off;
    a.user = d_user;
    a.S = m->mi_w + lay.at[kMindS];
    a.b0 = m->mi_w + lay.at[kMindB0];
    a.Wc = m->mi_w + lay.at[kMindWc];
    a.Wu = m->mi_w + lay.at[kMindWu];
    a.b1 = m->mi_w + lay.at[kMindB1];
    a.W2 = m->mi_w + lay.at[kMindW2];
    a.b2 = m->mi_w + lay.at[kMindB2];
    a.out = d_out;
    a.d_user = m->d_user;
    a.d_out = m->mi_dout;
    a.K = m->n_out;
    a.n_iter = m->mi_iter;
    a.h1 = m->h1;
    a.normalize = m->mi_norm;
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)mind_kernel, kMindLds))) return rc;
    mind_kernel<<<n_req, 256, kMindLds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// What the four entry points check alike; kd: the depth of one interest's list (pg_mind_recall) or unused
static int mind_check(const char* who, const pg_ctx* ctx, const pg_model* m, const pg_table* seq_t, const pg_table* item_emb, uint32_t n_req,
                      uint32_t k, uint32_t* kd) {
    PG_REQUIRE(ctx && m && seq_t, "%s: NULL argument", who);
    PG_REQUIRE(m->kind == PG_MODEL_MIND, "%s: model is not MIND", who);
    PG_REQUIRE(seq_t->dim == kMindD, "%s: sequence table dim %u != 64", who, seq_t->dim);
    PG_REQUIRE(n_req >= 1 && n_req <= (uint32_t)kMaxQueries, "%s: n_req=%u must be in [1,%d]", who, n_req, kMaxQueries);
    if (!kd) return PG_OK;
    PG_REQUIRE(item_emb, "%s: NULL argument", who);
    PG_REQUIRE(item_emb->dim == m->mi_dout, "%s: item-embedding table dim %u != the model's d_out %u", who, item_emb->dim, m->mi_dout);
    PG_REQUIRE(k >= m->n_out && k / m->n_out <= 16384, "%s: k=%u over %u interests: a list holds floor(k / K) rows, 1..16384", who, k, m->n_out);
    *kd = k / m->n_out;
    return PG_OK;
}

// the host forms' sequences: offsets from 0 that do not descend, at most PG_MIND_MAX_SEQ entries each
static int mind_check_seqs(const char* who, const uint32_t* seq_rows, const uint32_t* seq_off, uint32_t n_req) {
    PG_REQUIRE(seq_off, "%s: NULL argument", who);
    PG_REQUIRE(seq_off[0] == 0, "%s: seq_offsets[0] must be 0", who);
    for (uint32_t r = 0; r < n_req; ++r) {
        PG_REQUIRE(seq_off[r + 1] >= seq_off[r], "%s: seq_offsets not monotone at %u", who, r);
        PG_REQUIRE(seq_off[r + 1] - seq_off[r] <= kMindSeq, "%s: request %u has a sequence of %u rows, at most %u", who, r,
                   seq_off[r + 1] - seq_off[r], kMindSeq);
    }
    PG_REQUIRE(seq_off[n_req] == 0 || seq_rows, "%s: NULL argument", who);
    return PG_OK;
}

// a host form's inputs in the staging slot, behind whatever `more` takes first
struct MindStaged {
    float* user;
    uint32_t *seq_rows, *seq_off;
};
static void mind_take_inputs(Carve& c, const pg_model* m, uint32_t n_req, uint32_t n_seq, MindStaged* s) {
    s->user = c.take<float>((size_t)n_req * m->d_user);
    s->seq_rows = c.take<uint32_t>(n_seq ? n_seq : 1);
    s->seq_off = c.take<uint32_t>((size_t)n_req + 1);
}
static int mind_copy_inputs(pg_ctx* ctx, const pg_model* m, const MindStaged& s, const float* user, const uint32_t* seq_rows, const uint32_t* seq_off,
                            uint32_t n_req) {
    PG_HIP(hipMemcpyAsync(s.user, user, (size_t)n_req * m->d_user * 4, hipMemcpyHostToDevice, ctx->stream));
    if (seq_off[n_req]) PG_HIP(hipMemcpyAsync(s.seq_rows, seq_rows, (size_t)seq_off[n_req] * 4, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipMemcpyAsync(s.seq_off, seq_off, ((size_t)n_req + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    return PG_OK;
}

// pg_mind_recall[_dev] under the locks: floor(256 / K) requests per pass — their K interests into d_q, then one verified recall of
// (requests x K) queries at depth kd, whose [query][kd] output is the [request][interest][kd] layout.  Ends synchronised.
static int mind_recall_locked(pg_ctx* ctx, const pg_model* m, const pg_table* seq_t, const pg_table* item_emb, const float* d_user,
                              const uint32_t* d_seq_rows, const uint32_t* d_seq_off, uint32_t n_req, uint32_t kd, float* d_q, uint64_t* d_rows,
                              float* d_sc, uint32_t* out_count) {
    const uint32_t K = m->n_out, per = (uint32_t)kMaxQueries / K;
    for (uint32_t r0 = 0; r0 < n_req; r0 += per) {
        const uint32_t nr = std::min(per, n_req - r0);
        int rc;
        if ((rc = mind_interests_locked(ctx, m, seq_t, d_user + (size_t)r0 * m->d_user, d_seq_rows, d_seq_off + r0, nr, d_q))) return rc;
        if ((rc = recall_dev_locked(ctx, item_emb, d_q, nr * K, kd, d_rows + (size_t)r0 * K * kd, d_sc + (size_t)r0 * K * kd,
                                    out_count ? out_count + (size_t)r0 * K : nullptr, nullptr)))
            return rc;
    }
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_mind_interests_dev(pg_ctx* ctx, const pg_model* m, const pg_table* seq_table, const float* d_user_vecs, const uint32_t* d_seq_rows,
                          const uint32_t* d_seq_offsets, uint32_t n_req, float* d_out_interests) {
    int rc;
    if ((rc = pg::mind_check("pg_mind_interests_dev", ctx, m, seq_table, nullptr, n_req, 0, nullptr))) return rc;
    PG_REQUIRE(d_user_vecs && d_seq_offsets && d_out_interests, "pg_mind_interests_dev: NULL argument");      // (d_seq_rows may be NULL)
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(seq_table->rw);
    return pg::mind_interests_locked(ctx, m, seq_table, d_user_vecs, d_seq_rows, d_seq_offsets, n_req, d_out_interests);
}

int pg_mind_interests(pg_ctx* ctx, const pg_model* m, const pg_table* seq_table, const float* user_vecs, const uint32_t* seq_rows,
                      const uint32_t* seq_offsets, uint32_t n_req, float* out_interests) {
    int rc;
    if ((rc = pg::mind_check("pg_mind_interests", ctx, m, seq_table, nullptr, n_req, 0, nullptr))) return rc;
    PG_REQUIRE(user_vecs && out_interests, "pg_mind_interests: NULL argument");
    if ((rc = pg::mind_check_seqs("pg_mind_interests", seq_rows, seq_offsets, n_req))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(seq_table->rw);
    pg::MindStaged s;
    float* d_out;
    const size_t ob = (size_t)n_req * m->n_out * m->mi_dout;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& c) {
            d_out = c.take<float>(ob);
            pg::mind_take_inputs(c, m, n_req, seq_offsets[n_req], &s);
        }))) return rc;
    if ((rc = pg::mind_copy_inputs(ctx, m, s, user_vecs, seq_rows, seq_offsets, n_req))) return rc;
    if ((rc = pg::mind_interests_locked(ctx, m, seq_table, s.user, s.seq_rows, s.seq_off, n_req, d_out))) return rc;
    PG_HIP(hipMemcpyAsync(out_interests, d_out, ob * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_mind_recall_dev(pg_ctx* ctx, const pg_model* m, const pg_table* seq_table, const pg_table* item_emb, const float* d_user_vecs,
                       const uint32_t* d_seq_rows, const uint32_t* d_seq_offsets, uint32_t n_req, uint32_t k, uint64_t* d_out_rows,
                       float* d_out_scores, uint32_t* out_count) {
    int rc;
    uint32_t kd;
    if ((rc = pg::mind_check("pg_mind_recall_dev", ctx, m, seq_table, item_emb, n_req, k, &kd))) return rc;
    PG_REQUIRE(d_user_vecs && d_seq_offsets && d_out_rows && d_out_scores, "pg_mind_recall_dev: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead2 tr(item_emb, seq_table);
    float* d_q;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& c) { d_q = c.take<float>((size_t)pg::kMaxQueries * m->mi_dout); }))) return rc;
    return pg::mind_recall_locked(ctx, m, seq_table, item_emb, d_user_vecs, d_seq_rows, d_seq_offsets, n_req, kd, d_q, d_out_rows, d_out_scores,
                                  out_count);
}

int pg_mind_recall(pg_ctx* ctx, const pg_model* m, const pg_table* seq_table, const pg_table* item_emb, const float* user_vecs,
                   const uint32_t* seq_rows, const uint32_t* seq_offsets, uint32_t n_req, uint32_t k, uint64_t* out_rows, float* out_scores,
                   uint32_t* out_count) {
    int rc;
    uint32_t kd;
    if ((rc = pg::mind_check("pg_mind_recall", ctx, m, seq_table, item_emb, n_req, k, &kd))) return rc;
    PG_REQUIRE(user_vecs && out_rows && out_scores, "pg_mind_recall: NULL argument");
    if ((rc = pg::mind_check_seqs("pg_mind_recall", seq_rows, seq_offsets, n_req))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead2 tr(item_emb, seq_table);
    pg::MindStaged s;
    float *d_q, *d_sc;
    uint64_t* d_rows;
    const size_t no = (size_t)n_req * m->n_out * kd;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& c) {
            d_q = c.take<float>((size_t)pg::kMaxQueries * m->mi_dout);
            d_rows = c.take<uint64_t>(no);
            d_sc = c.take<float>(no);
            pg::mind_take_inputs(c, m, n_req, seq_offsets[n_req], &s);
        }))) return rc;
    if ((rc = pg::mind_copy_inputs(ctx, m, s, user_vecs, seq_rows, seq_offsets, n_req))) return rc;
    if ((rc = pg::mind_recall_locked(ctx, m, seq_table, item_emb, s.user, s.seq_rows, s.seq_off, n_req, kd, d_q, d_rows, d_sc, out_count))) return rc;
    PG_HIP(hipMemcpyAsync(out_rows, d_rows, no * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(out_scores, d_sc, no * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

}  // extern "C"
