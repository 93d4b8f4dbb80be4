// recall.hip — exact inner-product top-K over an HBM-resident fp32 table.
//
// Replaces the reference's remote candidate generation: FaissModel.Run → VectorClient.Search
// (algorithm/faiss/model.go:29-31, vector_client.go:32-41) and Hologres'
// pm_approx_inner_product_distance ... ORDER BY distance desc LIMIT n
// (service/recall/hologres_vector_recall.go:23); call site service/recall/vector_recall.go:88-102.
//
// Specification:  score(row,q) = chain_{k asc} fmaf(x[row][k], q[k], acc), fp32 —
// exactly what gfx950's v_mfma_f32_32x32x2_f32 computes (a k-ordered fmaf chain, one rounding per
// step), so a request's scores do not depend on how many other requests share the table pass.
// Order: score descending (IEEE totalOrder, NaN last), then row ascending, via a 64-bit key.
//
// This file: the table pass — its kernels and their launchers (dispatch_scan, screen_launch, rescore_launch, ...), which own the
// choice of an instantiation and its grid.  Its siblings, sharing recall_shared.hpp:
//   recall_plan.hip    the plans that chain the launches (recall_job_prepare / enqueue / check / finish); their arithmetic: recall_plan_math.hpp
//   recall_select.hip  select_kernel, the final_* kernels, launch_select, final_launch, the top-k merge of per-shard lists
//   recall_table.hip   what is derived from a table, lazily: shadows, statistics, row norms, the threshold model
//   recall_filter.hip  row filters, the compaction of the admitted rows, filtered recalls and views
//   recall_entry.hip   recall_dev_locked, batching, the exclusion lists and the pg_* entry points
//
// Kernels
//   scan_kernel      HBM-bound.  One wave = one 32-row block at a time; rows stream HBM → LDS by
//                    LDS-DMA (global_load_lds_dwordx4, full 128-B lines, no VGPR staging) through a
//                    per-wave ring of 8 KiB pieces (no workgroup barriers); A fragments are read
//                    from LDS conflict-free thanks to a per-row rotation applied on the DMA's
//                    *source* address; 32 queries ride in the B operand.  Rows whose score reaches
//                    the query's running threshold are appended to a candidate list.
//   screen_kernel    the same walk over a quantised shadow of the rows (int8 at dim 128, bf16 at dim 64): an
//                    int8 / bf16 MFMA bounds every row·query score rigorously, pairs whose bound reaches the
//                    threshold are "suspects"; rescore_kernel scores the suspects exactly from the fp32 rows.
//                    Up to 256 queries per pass; results identical to scan_kernel's, bit for bit.
#include "common.hpp"
#include "recall_shared.hpp"

#include <type_traits>

namespace pg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// (kPieceRows = 32: recall_plan_math.hpp)
constexpr int kPieceCols = 32;                             // one 128-B line per row
constexpr int kPieceBytes = kPieceRows * kPieceCols * 4;   // 4 KiB
constexpr int kPieceDmas = kPieceBytes / 1024;             // LDS-DMA instructions per piece
constexpr int kPieceQuads = kPieceCols / 4;                // 16-B quads per row of a piece
constexpr int kRingSlots = 4;                              // per wave: 1 consumed + 3 in flight
constexpr int kScanWaves = 8;                              // waves per workgroup (2 per SIMD: one wave's
                                                           // waits/epilogues hide behind the other's MFMAs)
constexpr int kScanLdsRing = kScanWaves * kRingSlots * kPieceBytes;   // 128 KiB
constexpr int kStageCap = 280;                             // staged hits per wave (fills the LDS left by the ring)
constexpr int kStageBytes = kStageCap * 12 + 512;          // keys + query ids + 64 counters + 64 bases
constexpr int kScanLds = kScanLdsRing + kScanWaves * kStageBytes;


// Pilot sample: logical block L of a stride-S launch is table block slot*S + jitter(slot), where
// slot = L*mul mod n_slots is a fixed permutation of the n_slots sample slots (mul coprime with
// n_slots) and jitter < S.  The permutation makes the pilot's own streaming order independent of the
// table order (a table sorted by score would otherwise defeat its running threshold); the jitter keeps
// a periodic layout from aliasing with the sample.  S = 1 is the identity.
__device__ __forceinline__ uint32_t slot_block(uint32_t slot, uint32_t S) {
    return slot * S + (uint32_t)(((uint64_t)(slot * 2654435761u) * S) >> 32);       // jitter in [0, S)
}
__device__ __forceinline__ uint32_t sample_block(uint32_t L, uint32_t S, uint32_t mul, uint32_t mod) {
    if (S == 1) return L;
    return slot_block((uint32_t)(((uint64_t)L * mul) % mod), S);
}

// One LDS-DMA instruction (64 lanes x 16 B = 1 KiB): global → LDS without touching VGPRs.
// `base` is the wave-uniform byte address of the piece (first row, first column of the piece),
// `voff` the lane's byte offset, `lds_addr` the wave-uniform LDS destination (the hardware adds
// lane*16).  M0 carries the LDS address; it is saved/restored because hipcc owns it outside this
// asm.  (The instruction's immediate offset is NOT used: on an LDS-DMA it is added to the LDS
// address too.)  `nt`: the table is streamed once, keep it out of the way of L2-resident data.
//
// WAR guard: `after` must be a value returned by a ds_read of the piece CURRENTLY being computed.
// It is an (unused) input of the asm, so hipcc waits for that read before the DMA issues; LDS
// returns in order, hence every read of the previous piece — whose slot this DMA overwrites — has
// completed too.  Without it a DMA served from L2/MALL was observed to land before a still-queued
// ds_read of the old piece (1 lost candidate in ~10 % of small-table runs).
__device__ __forceinline__ void dma_one(const char* base, uint32_t lds_addr, uint32_t voff, float after) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2 nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(base), "s"(lds_addr), "v"(after)
        : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// NQB = number of 32-query column blocks riding in the B operand (1: up to 32 queries, 2: up to 64).
// With two blocks every A fragment feeds two independent accumulator chains and the kernel becomes
// fp32-MFMA-bound instead of HBM-bound (2 x 64 cycles per 32 B of table per SIMD).
// L2: the candidates are the rows of SMALLEST squared Euclidean distance (service/recall/hologres_vector_recall_v2.go:23).  The
// inner products come out of the same MFMA chains; every accumulator is then turned into -d = fmaf(2, ip, -(|x|^2 + |q|^2))
// — the block's 32 row norms arrive by scalar loads (the block's first row is wave-uniform; lgkmcnt, not the ring's vmcnt) —
// and everything behind (threshold streaming, keys, select, final) works on -d unchanged.  HBM-bound like the exact scan.
// (VAR is kept only so that the kernel's name stays the same)
template <int DIM, int NQB = 1, int VAR = 0, bool L2 = false>
__global__ __launch_bounds__(64 * kScanWaves, 2) void scan_kernel(ScanArgs a) {
    static_assert(VAR == 0);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PPB = DIM / kPieceCols;       // pieces per 32-row block
    constexpr int NS = kRingSlots;
    constexpr int ND = kPieceDmas;              // 4
    constexpr int NQ = kPieceQuads;             // 8
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t gw = blockIdx.x * kScanWaves + wave;
    const uint32_t W = gridDim.x * kScanWaves;
    const int i32 = lane & 31;       // row within block (A), query (B, C)
    const int h = lane >> 5;         // k parity (A, B); row half (C)
    if (a.group_q) {                 // this workgroup's query group
        const uint32_t g0 = blockIdx.y * a.group_q;
        a.qpad += (size_t)g0 * DIM;
        a.thr += g0;
        a.cnt += g0;
        a.cand += (uint64_t)g0 * a.cap;
        if (L2) a.nqv += g0;
        a.nq = a.nq - g0 < a.group_q ? a.nq - g0 : a.group_q;
    }

    // B operand: bq[s] = Q[query = lane&31][k = 2s + h]
    float bq[NQB][DIM / 2];
    float thr[NQB];
    float nq2[NQB];                  // L2: |q|^2 of this lane's query
    bool active[NQB];
#pragma unroll
    for (int c = 0; c < NQB; ++c) {
#pragma unroll
        for (int s = 0; s < DIM / 2; ++s) bq[c][s] = a.qpad[(c * 32 + i32) * DIM + 2 * s + h];
        thr[c] = a.thr[c * 32 + i32];
        active[c] = (uint32_t)(c * 32 + i32) < a.nq;
        nq2[c] = (L2 && active[c]) ? a.nqv[c * 32 + i32] : 0.0f;
        if (L2) asm volatile("" : "+v"(nq2[c]));
    }
    // Pin the operand loads' completion HERE: hipcc places a load's s_waitcnt at its first use,
    // which would otherwise land inside the streaming loop as vmcnt(0) and drain the DMA ring.
#pragma unroll
    for (int c = 0; c < NQB; ++c) {
#pragma unroll
        for (int s = 0; s < DIM / 2; ++s) asm volatile("" : "+v"(bq[c][s]));
        asm volatile("" : "+v"(thr[c]));
    }

    // DMA lane offsets.  A piece is 32 rows x 32 columns (one 128-B line per row); DMA n covers
    // LDS quad slots S = n*64 + lane ↔ (row i = S/8, quad p = S%8), which receive global quad
    // (p + i/2) % 8 of that row: the rotation makes the A-fragment ds_read_b128 conflict-free.
    uint32_t voff[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int S = n * 64 + lane;
        const int i = S >> 3, p = S & 7;
        voff[n] = (uint32_t)(i * DIM + 4 * ((p + (i >> 1)) & 7)) * 4u;
    }
    const uint32_t lds_wave_u = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + wave * (NS * kPieceBytes));
    char* const lds_ptr = smem + wave * (NS * kPieceBytes);
    const int rd_row = i32 * 128;
    const int rd_rot = (i32 >> 1) * 16;

    // each wave walks a CONTIGUOUS run of row blocks (sequential 16 KiB reads), runs are spread
    // evenly over the launch's waves
    const uint32_t total = a.rb_end - a.rb_begin;
    const uint32_t bpw = (total + W - 1) / W;
    const uint32_t first = gw * bpw;
    const uint32_t nblk = first < total ? (total - first < bpw ? total - first : bpw) : 0;
    if (nblk == 0) return;

    // wave-uniform source base and LDS destination of piece t (tail pieces re-read the last block)
    auto piece_addr = [&](uint32_t t, const char*& ub, uint32_t& dst) {
        uint32_t b = t / PPB;
        if (b >= nblk) b = nblk - 1;
        const uint64_t rb = sample_block(a.rb_begin + first + b, a.stride, a.perm_mul, a.perm_mod);
        const char* base = (const char*)a.tab + rb * (uint64_t)(kPieceRows * DIM * 4) + (t % PPB) * (kPieceCols * 4);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)(uintptr_t)base >> 32));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)base);
        ub = (const char*)(((uint64_t)hi << 32) | lo);
        dst = lds_wave_u + __builtin_amdgcn_readfirstlane(t % NS) * kPieceBytes;
    };

    // wave-private staging list for threshold hits (keys + query ids)
    uint64_t* const st_key = reinterpret_cast<uint64_t*>(smem + kScanLdsRing + wave * kStageBytes);
    uint32_t* const st_q = reinterpret_cast<uint32_t*>(st_key + kStageCap);
    uint32_t* const st_cnt = st_q + kStageCap;            // [64] per-query counts / running offsets
    uint32_t* const st_base = st_cnt + 64;                // [64] reserved base per query
    uint32_t st_n = 0;
    // Flush: reserve space per QUERY (<= 64 returning global atomics per flush instead of one per
    // hit — the list counters are the hottest words of the launch), then scatter.
    auto flush = [&]() {
        st_cnt[lane] = 0;
        for (uint32_t e0 = 0; e0 < st_n; e0 += 64) {
            const uint32_t e = e0 + lane;
            if (e < st_n) atomicAdd(&st_cnt[st_q[e]], 1u);
        }
        {
            const uint32_t c = st_cnt[lane];
            st_base[lane] = c ? atomicAdd(&a.cnt[lane], c) : 0u;
            st_cnt[lane] = 0;
        }
        for (uint32_t e0 = 0; e0 < st_n; e0 += 64) {
            const uint32_t e = e0 + lane;
            if (e < st_n) {
                const uint32_t q = st_q[e];
                const uint32_t pos = st_base[q] + atomicAdd(&st_cnt[q], 1u);
                if (pos < a.cap) a.cand[(uint64_t)q * a.cap + pos] = st_key[e];
                else *a.overflow = 1u;
            }
        }
        st_n = 0;
        __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0), visible to hipcc's bookkeeping
    };

    // prologue: pieces 0..NS-2 in flight
#pragma unroll
    for (int t = 0; t < NS - 1; ++t) {
        const char* src;
        uint32_t dst;
        piece_addr(t, src, dst);
#pragma unroll
        for (int n = 0; n < ND; ++n) dma_one(src, dst + n * 1024, voff[n], 0.0f);
    }

    for (uint32_t b = 0; b < nblk; ++b) {
        f32x16 acc[NQB];
#pragma unroll
        for (int c = 0; c < NQB; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
#pragma unroll
        for (int pc = 0; pc < PPB; ++pc) {
            const uint32_t t = b * PPB + pc;
            // pieces t..t+NS-2 are in flight (ND DMAs each); piece t+NS-1 is issued below, one DMA
            // every other quad, into the slot that piece t-1 just vacated
            wait_vmcnt<ND * (NS - 2)>();                    // piece t has landed
            const char* nb_src;
            uint32_t nb_dst;
            piece_addr(t + NS - 1, nb_src, nb_dst);
            const char* slot = lds_ptr + (t % NS) * kPieceBytes + rd_row;
            // all of the piece's A-fragment reads are issued up front (8 x ds_read_b128 in flight),
            // so LDS latency is paid once per piece instead of once per quad
            f32x4 qv[NQ];
#pragma unroll
            for (int g = 0; g < NQ; ++g)
                qv[g] = *reinterpret_cast<const f32x4*>(slot + ((g * 16 - rd_rot) & 112));
            __builtin_amdgcn_sched_barrier(0);      // keep the reads up here (hipcc would sink them to their uses)
#pragma unroll
            for (int g = 0; g < NQ; ++g) {
                const f32x4 q = qv[g];
                if (g < ND) dma_one(nb_src, nb_dst + g * 1024, voff[g], q.x);
                const float a0 = h ? q.y : q.x;
                const float a1 = h ? q.w : q.z;
                const int s = pc * (kPieceCols / 2) + 2 * g;
#pragma unroll
                for (int c = 0; c < NQB; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bq[c][s], acc[c], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NQB; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bq[c][s + 1], acc[c], 0, 0, 0);
            }
        }
        if constexpr (L2) {
            const uint32_t l2_row0 = __builtin_amdgcn_readfirstlane(
                sample_block(a.rb_begin + first + b, a.stride, a.perm_mul, a.perm_mod) * kPieceRows);
            const float* const nxp = a.nx + l2_row0;               // wave-uniform: scalar loads
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                const float nxa = nxp[ro], nxb = nxp[ro + 4];
                const float nxr = h ? nxb : nxa;
#pragma unroll
                for (int c = 0; c < NQB; ++c) acc[c][r] = __fmaf_rn(2.0f, acc[c][r], -(nxr + nq2[c]));
            }
        }
        // ---- threshold test: C layout col = lane&31 (query within its block), row = (r&3)+8*(r>>2)+4*h.
        // Fast path: one not-less-than compare per accumulator register, OR-reduced.
        bool any = false;
#pragma unroll
        for (int c = 0; c < NQB; ++c) {
            bool anyc = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) anyc |= !(acc[c][r] < thr[c]);
            any |= anyc && active[c];
        }
        if (__builtin_amdgcn_ballot_w64(any) != 0) {
            // Hits are rare (≈ K/rows_seen per row·query), so they are parked in a wave-private LDS
            // staging list and flushed in bulk: a returning atomic costs a full vmcnt drain of the
            // DMA ring, which must not happen once per block.
            const uint32_t row0 = sample_block(a.rb_begin + first + b, a.stride, a.perm_mul, a.perm_mod) * kPieceRows;
#pragma unroll
            for (int c = 0; c < NQB; ++c) {
                const uint32_t qid = (uint32_t)(c * 32 + i32);
                uint32_t pass = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const bool p = active[c] && !(acc[c][r] < thr[c]) && row < a.row_end && row_filter_pass(a.filter, row < a.row_end ? row : 0u);
                    pass |= (p ? 1u : 0u) << r;
                }
                if (__builtin_amdgcn_ballot_w64(pass != 0) == 0) continue;
                uint32_t total_hits = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    total_hits += __popcll(__builtin_amdgcn_ballot_w64((pass >> r) & 1u));
                if (st_n + total_hits > (uint32_t)kStageCap) flush();
                if (total_hits > (uint32_t)kStageCap) {
                    // dense case (first chunk: threshold still -inf): straight to global memory
                    if (pass != 0) {
                        uint32_t pos = atomicAdd(&a.cnt[qid], (uint32_t)__popc(pass));
                        uint64_t* dst = a.cand + (uint64_t)qid * a.cap;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            if (pass & (1u << r)) {
                                const uint32_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                                if (pos < a.cap) dst[pos] = topk_key(acc[c][r], row);
                                else *a.overflow = 1u;
                                ++pos;
                            }
                        }
                    }
                    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to hipcc's bookkeeping
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool p = (pass >> r) & 1u;
                        const uint64_t m = __builtin_amdgcn_ballot_w64(p);
                        if (m != 0) {
                            if (p) {
                                const uint32_t pos = st_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                                const uint32_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                                st_key[pos] = topk_key(acc[c][r], row);
                                st_q[pos] = qid;
                            }
                            st_n += __popcll(m);
                        }
                    }
                }
            }
        }
    }
    flush();
    wait_vmcnt<0>();   // drain the tail re-reads before the wave's LDS is released
}

// ---------------------------------------------------------------------------------------------
// Screened scan: the same stream, but the per-row scores are first *bounded* with bf16 MFMA and
// only rows that could beat the threshold are re-scored exactly.
//
//   s~ = sum_k bf16(x_k) * bf16(q_k)   (v_mfma_f32_32x32x16_bf16, 16x cheaper than the fp32 MFMA)
//   |s~ - s| <= eps_q = 0.008 * max_row_norm * ||q||          (s = the specification's fmaf chain)
//     [2*2^-8 + 2^-16 operand rounding (any rounding mode) + 2 * 128 * 2^-24 accumulation, times
//      sum|x_k q_k| <= ||x||*||q||]
// A row is staged when !(s~ < thr_q - eps_q); at flush time every staged (row, query) pair gets the
// exact k-ascending fmaf chain from the fp32 table and is kept only if !(s < thr_q).  Any member of
// the final top-K has s >= thr_q at every moment (thr is a lower bound of the final K-th score), so
// s~ >= thr_q - eps_q and it is staged: the result is identical, bit for bit, to the exact scan.
// With 128 queries (4 column blocks) per pass the MFMA work is 1/4 of the 32-query exact kernel's
// and the kernel stays HBM-bound.
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

constexpr int kScreenLds = 163840;              // the whole LDS of a CU: ring (128 KiB) + staging (32 KiB)

// (ScanArgs, ScreenArgs: recall_shared.hpp)
// Hit records (query halves; kRecBytes = 48, recall_plan_math.hpp).  A 32-row x 16-query tile with a suspect in it has, as a rule, exactly one: one lane, one of
// its 8 accumulators (two row halves x 4 registers of v_mfma_i32_16x16x64_i8).  Finding the register inside the scan kernel —
// compare / add-with-carry pairs and a staging loop, issued for the whole wave on behalf of that one lane — cost about as
// many VALU slots as the reject test itself.  Instead the lane parks its 8 accumulators as they are (32 B) with a tag (first
// row of the block; query | lane group << 8) in the wave's LDS staging area and moves on: three LDS writes under the hit
// lanes' exec mask.  (On the 32x32x32 shape the record was a lane's 16 accumulators + tag, 80 B.)  Every
// kRecStage records the area is copied to the wave's region of a global record buffer (plain coalesced stores, no
// atomics, no wait: the stores add to vmcnt, which only makes the ring's counted waits conservative for a moment —
// loads return in order among themselves).  screen_decode_kernel then does the compares with one record per lane — all
// 64 lanes busy — and fills the per-query suspect lists that rescore_kernel reads.  (Stores straight from the hit path,
// without the LDS stage, were measured: 4.35 vs 3.1 ms per pass — with stores in flight in every second block the
// counted waits over-wait all the time and the ring runs one piece deep.)

// NQB query blocks of 32; WAVES waves per workgroup.  <=128 queries: 8 waves (2 per SIMD), ring of 4
// pieces per wave; 256 queries: the 256 B-operand registers leave room for one wave per SIMD only, so
// 4 waves with a ring of 8 pieces each.
// I8: the shadow and the queries are int8 and the bound is an exact int32 dot product on
// v_mfma_i32_32x32x32_i8 — same issue rate as the bf16 MFMA at twice the k per instruction, over half the
// bytes per row.
// QH: query halves — the wave serves NQB x QH query blocks of 32, QH groups of NQB one after the other on the same table
// block, re-using the accumulators (int8, 256 queries: 2 x 4 blocks in 8 waves — two waves per SIMD, so one
// wave's test, hit path and DMA issue run under the other's MFMAs; all 128 B-operand registers in the AGPR half).
// This path runs on v_mfma_i32_16x16x64_i8 — a half is 8 column blocks of 16 queries x 2 row halves — at the same
// operations per cycle as 32x32x32 and a higher clock under the package power cap (DESIGN.md §4.1a, Appendix A;
// scripts/micro/mfma_shape_i8.hip): its own A read pattern, DMA rotation, B packing (screen_prep8_kernel) and record.
// (SPLIT and VAR are kept only so that the kernel's name stays the same)
template <int DIM, int NQB, int WAVES, int SPLIT = 1, int VAR = 0, bool I8 = false, int QH = 1, int L2 = 0>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void screen_kernel(ScreenArgs a) {
    static_assert(SPLIT == 1 && VAR == 0);
    static_assert(!L2 || (I8 && QH == 1), "squared-Euclidean screen: the int8 kernels of <= 128 queries");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the kernel streams the table's shadow: a piece is 32 rows x one 128-B line per row (64 bf16 / 128 int8)
    constexpr int EB = I8 ? 1 : 2;               // bytes per shadow element
    constexpr int kCols16 = 128 / EB;
    static_assert(DIM % kCols16 == 0, "a shadow row is a whole number of 128-B lines");
    constexpr int PPB = DIM / kCols16;           // pieces per 32-row block (1 or 2)
    constexpr int NS = kScanLdsRing / (WAVES * kPieceBytes);        // ring slots per wave
    constexpr int ND = kPieceDmas;
    constexpr int KS = DIM * EB / 32;            // k-steps: 16 bf16 or 32 int8 (32 B of a row) each
    typedef int i32x16 __attribute__((ext_vector_type(16)));
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    using AccT = typename std::conditional<I8, i32x16, f32x16>::type;
    using ThrT = typename std::conditional<I8, int, float>::type;
    // (query halves: the last two B fragments sit in LDS — 2 KiB for the workgroup — because the allocator wants a
    // few registers of the AGPR half for itself and would otherwise bring two fragments back from scratch per block,
    // behind an s_waitcnt vmcnt(0) that also drains the DMA ring)
    // (query halves, 16x16x64: a lane has 16 query columns, and 16 threshold registers do not fit beside 64 accumulators at
    // 128 arch registers — the 256 integer thresholds follow the two fragments, eight ds_read_b32 per half under 512 MFMA cycles)
    constexpr int kBLds = QH > 1 ? 3072 : 0;
    constexpr int kStageBytesW = (kScreenLds - kScanLdsRing - kBLds) / WAVES;
    constexpr int NQT = NQB * QH;                // query blocks of this wave
    static_assert(QH == 1 || PPB == 1, "query halves: one piece per block");
    constexpr int kCap = (kStageBytesW - NQT * 256 - 16) / 8;       // staged (row, query) pairs per wave
    constexpr int kScanWaves = WAVES;            // (shadows the exact kernel's constant in this scope)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t gw = blockIdx.x * kScanWaves + wave;
    const uint32_t W = gridDim.x * kScanWaves;
    const int i32 = lane & 31;
    const int h = lane >> 5;

    // B operand: bfrag[c][ks] = Q[c*32 + (lane&31)][ks*16 + 8h .. +7] as bf16
    uint4 bfrag[NQT][KS];
    ThrT thr_s[NQT];
    float eu[NQT];                                    // bf16: eps_unit of this lane's query, per query block
    float la[NQT];                                    // L2: A_q
    bool active[NQT];
    char* const b_lds = smem + kScreenLds - kBLds;
    int* const thr_lds = reinterpret_cast<int*>(b_lds + 2048);
    if constexpr (QH > 1) {
        if (wave == 0) {
            *reinterpret_cast<uint4*>(b_lds + lane * 16) = a.qb16[((NQT - 1) * KS + KS - 2) * 64 + lane];
            *reinterpret_cast<uint4*>(b_lds + 1024 + lane * 16) = a.qb16[((NQT - 1) * KS + KS - 1) * 64 + lane];
        }
        if (threadIdx.x < (uint32_t)kMaxQueries)      // (inactive columns: never a suspect)
            thr_lds[threadIdx.x] = threadIdx.x < a.nq ? __float_as_int(a.thr_screen[threadIdx.x]) : 0x7fffffff;
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NQT; ++c) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (QH > 1 && c == NQT - 1 && ks >= KS - 2) bfrag[c][ks] = make_uint4(0, 0, 0, 0);     // (in LDS; unused)
            else bfrag[c][ks] = a.qb16[(c * KS + ks) * 64 + lane];
        }
        active[c] = (uint32_t)(c * 32 + i32) < a.nq;
        if constexpr (QH > 1) thr_s[c] = 0;                // (query halves: the thresholds are in LDS, by 16-query block)
        else if constexpr (I8) thr_s[c] = active[c] ? __float_as_int(a.thr_screen[c * 32 + i32]) : 0x7fffffff;
        else thr_s[c] = active[c] ? a.thr_screen[c * 32 + i32] : __builtin_inff();
        eu[c] = (!I8 && active[c]) ? a.eps_unit[c * 32 + i32] : 0.0f;
        if constexpr (L2 != 0) {                      // A_q in la, B_q in eu (L2 = 2: C'_q and 2 s_x s_q; inactive columns: never a suspect)
            la[c] = active[c] ? a.thr_screen[c * 32 + i32] : __builtin_inff();
            eu[c] = active[c] ? a.l2_b[c * 32 + i32] : 0.0f;
        }
    }
#pragma unroll
    for (int c = 0; c < NQT; ++c) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (QH > 1 && c == NQT - 1 && ks >= KS - 2) continue;
            if (NQT > 4)     // >= 128 B registers: park them in the AGPR half, where the MFMA reads them directly
                asm volatile("" : "+a"(bfrag[c][ks].x), "+a"(bfrag[c][ks].y), "+a"(bfrag[c][ks].z), "+a"(bfrag[c][ks].w));
            else
                asm volatile("" : "+v"(bfrag[c][ks].x), "+v"(bfrag[c][ks].y), "+v"(bfrag[c][ks].z), "+v"(bfrag[c][ks].w));
        }
        if (QH == 1) asm volatile("" : "+v"(thr_s[c]));
        if (!I8 || L2) asm volatile("" : "+v"(eu[c]));
        if (L2) asm volatile("" : "+v"(la[c]));
    }

    uint32_t voff[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int S = n * 64 + lane;
        const int i = S >> 3, p = S & 7;
        // row i, rotated 16-B quad p.  A ds_read_b128 lane group ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of a wave half) must
        // cover the 64 banks once.  32x32 shapes: the group reads 16 rows at ONE quad — rotate by i >> 1.  16x16x64 (query
        // halves): it reads rows {0-3, 12-15} at quad q and rows 4-11 at q +- 1 — rotate by i & 6 (row pairs at q - {0, 2, 4, 6,
        // 0, 2, 4, 6}; with the +-1 of pairs 2-5 all eight differ, where i >> 1 collides two-way: measured, scripts/micro/mfma_shape_i8.hip)
        voff[n] = (uint32_t)(i * DIM * EB + 16 * ((p + (QH > 1 ? (i & 6) : (i >> 1))) & 7));
    }
    const uint32_t lds_wave_u = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + wave * (NS * kPieceBytes));
    char* const lds_ptr = smem + wave * (NS * kPieceBytes);
    const int rd_row = i32 * 128;
    const int rd_rot = (i32 >> 1) * 16;

    const uint32_t total = a.rb_end - a.rb_begin;
    uint32_t first, nblk;
    if (WAVES == 8 && a.early_share != 512) {
        // Two waves per SIMD (w and w + 4), and the SIMD's arbiter favours the older one: per-phase cycle counts of the
        // 256-query kernel had waves 0-3 finish an equal share in 78 % of the time of waves 4-7, which then ran the last fifth
        // of the launch alone — one wave per SIMD, nothing to overlap with.  So the pair's run of blocks is split unevenly
        // (early_share / 1024 of it to the early wave) and both finish together.
        const uint32_t P = gridDim.x * 4;
        const uint32_t pb = (total + P - 1) / P;
        const uint32_t pbase = (blockIdx.x * 4 + (wave & 3)) * pb;
        const uint32_t pend = pbase + pb < total ? pbase + pb : total;
        uint32_t cut = pbase + (uint32_t)(((uint64_t)pb * a.early_share + 512) >> 10);
        if (cut > pend) cut = pend;
        first = wave < 4 ? pbase : cut;
        const uint32_t last = wave < 4 ? cut : pend;
        nblk = first < last ? last - first : 0;
    } else {
        const uint32_t bpw = (total + W - 1) / W;
        first = gw * bpw;
        nblk = first < total ? (total - first < bpw ? total - first : bpw) : 0;
    }
    if (nblk == 0) {
        if (QH > 1 && lane == 0) a.rec_cnt[gw] = 0;
        return;
    }

    // Physical table block of each logical block this wave walks, kept D blocks ahead of the one being
    // scored (the DMA ring runs NS-1 pieces ahead).  Incremental: slot += mul (mod n_slots) per block
    // for a pilot sample, +1 for a full pass — no division in the loop.  Blocks past the end of the
    // run repeat the last one (tail pieces re-read it; they are never scored).
    // (Tried for the query halves: the next piece sent into the slot just READ — its four fragments are in registers at the top
    // of the iteration — i.e. the whole ring, NS pieces = 128 KiB per CU, in flight instead of NS - 1: 311 vs 318 M items/s.
    // More requests in flight than the memory pipeline queues only stall the wave at the DMA issue.)
    constexpr int D = (PPB - 1 + NS - 1) / PPB;
    const bool strided = a.stride != 1;
    const uint32_t L0 = a.rb_begin + first;
    uint32_t walk_slot = strided ? (uint32_t)(((uint64_t)L0 * a.perm_mul) % a.perm_mod) : L0;
    uint32_t walk_n = 0;                          // logical blocks handed out so far
    auto next_phys = [&]() -> uint32_t {
        const uint32_t ph = strided ? slot_block(walk_slot, a.stride) : walk_slot;
        if (walk_n + 1 < nblk) {
            ++walk_n;
            if (strided) {
                walk_slot += a.perm_mul;
                if (walk_slot >= a.perm_mod) walk_slot -= a.perm_mod;
            } else {
                ++walk_slot;
            }
        }
        return __builtin_amdgcn_readfirstlane(ph);
    };
    uint32_t phys[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) phys[j] = next_phys();
    // wave-uniform source base and LDS destination of piece `pc_abs` pieces after the start of the
    // block being scored (compile-time offset), global piece counter t for the ring slot
    auto piece_addr = [&](int rel_piece, uint32_t t, const char*& ub, uint32_t& dst) {
        const uint32_t ph = phys[rel_piece / PPB];
        const char* base = (const char*)a.tab16 + (uint64_t)ph * (uint64_t)(kPieceRows * DIM * EB) + (rel_piece % PPB) * 128;
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)(uintptr_t)base >> 32));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)base);
        ub = (const char*)(((uint64_t)hi << 32) | lo);
        dst = lds_wave_u + __builtin_amdgcn_readfirstlane(t % NS) * kPieceBytes;
    };

    // staging: (row, query) pairs that passed the screen ("suspects").  They are parked in a
    // wave-private LDS list and flushed in bulk into per-query global suspect lists; the exact
    // re-scoring runs afterwards in rescore_kernel, with the whole chip hiding the gather latency
    // (done here it cost one dependent HBM round trip chain per 64 suspects per wave).
    uint32_t* const st_row = reinterpret_cast<uint32_t*>(smem + kScanLdsRing + wave * kStageBytesW);
    uint32_t* const st_q = st_row + kCap;
    uint32_t* const st_cnt = st_q + kCap;                 // [NQT*32]
    uint32_t* const st_base = st_cnt + NQT * 32;          // [NQT*32]
    uint32_t st_n = 0;
    auto flush = [&]() {
        // per-query reservation (one returning atomic per query present), then scatter the row ids
#pragma unroll
        for (int part = 0; part < (NQT + 1) / 2; ++part)
            if (lane + 64 * part < NQT * 32) st_cnt[lane + 64 * part] = 0;
        for (uint32_t e0 = 0; e0 < st_n; e0 += 64) {
            const uint32_t e = e0 + lane;
            if (e < st_n) atomicAdd(&st_cnt[st_q[e]], 1u);
        }
#pragma unroll
        for (int part = 0; part < (NQT + 1) / 2; ++part) {
            const int q = lane + 64 * part;
            if (q < NQT * 32) {
                const uint32_t c = st_cnt[q];
                st_base[q] = c ? atomicAdd(&a.susp_cnt[q], c) : 0u;
                st_cnt[q] = 0;
            }
        }
        for (uint32_t e0 = 0; e0 < st_n; e0 += 64) {
            const uint32_t e = e0 + lane;
            if (e < st_n) {
                const uint32_t q = st_q[e];
                const uint32_t pos = st_base[q] + atomicAdd(&st_cnt[q], 1u);
                if (pos < a.cap) a.susp[(uint64_t)q * a.cap + pos] = st_row[e];
                else *a.overflow = 1u;
            }
        }
        st_n = 0;
        __builtin_amdgcn_s_waitcnt(0x0F70);
    };

#pragma unroll
    for (int t = 0; t < NS - 1; ++t) {
        const char* src;
        uint32_t dst;
        piece_addr(t, t, src, dst);
#pragma unroll
        for (int n = 0; n < ND; ++n) dma_one(src, dst + n * 1024, voff[n], 0.0f);
    }

    if constexpr (QH > 1) {
        // hit records: staged in LDS (the area the other variants stage (row, query) pairs in), flushed to this wave's region
        constexpr uint32_t kRecStage = (uint32_t)kStageBytesW / kRecBytes;
        char* const rec_lds = smem + kScanLdsRing + wave * kStageBytesW;
        char* const rec_glb = a.rec + (size_t)gw * a.rec_cap * kRecBytes;
        uint32_t rec_st = 0, rec_total = 0;
        const int r16 = lane & 15, g16 = lane >> 4;
        const int rot16 = (r16 & 6) * 16;
        const uint32_t tag16 = (uint32_t)r16 | ((uint32_t)g16 << 8);      // a record's tag word: query | lane group << 8
        auto rec_flush = [&]() {
            if (rec_total + rec_st > a.rec_cap) {
                // region full (the table's best rows sit together): the staged records go to the shared pool — one returning
                // atomic, which also drains the ring; rare by construction.  A full pool fails the plan (the caller falls back).
                uint32_t g = 0;
                if (lane == 0) g = atomicAdd(&a.rec_cnt[a.rec_waves], rec_st);
                g = __builtin_amdgcn_readfirstlane(g);
                if (g + rec_st > a.rec_pool_cap) {
                    if (lane == 0) { *a.overflow = 1u; a.overflow[kRecOvfWord] = 1u; }
                } else {
                    char* const dst = a.rec_pool + (size_t)g * kRecBytes;
                    for (uint32_t o = lane * 16; o < rec_st * kRecBytes; o += 1024)
                        *reinterpret_cast<i32x4*>(dst + o) = *reinterpret_cast<const i32x4*>(rec_lds + o);
                }
            } else {
                char* const dst = rec_glb + (size_t)rec_total * kRecBytes;
                for (uint32_t o = lane * 16; o < rec_st * kRecBytes; o += 1024)
                    *reinterpret_cast<i32x4*>(dst + o) = *reinterpret_cast<const i32x4*>(rec_lds + o);
                rec_total += rec_st;
            }
            rec_st = 0;
        };
        for (uint32_t b = 0; b < nblk; ++b) {
            wait_vmcnt<ND * (NS - 2)>();
            const char* nb_src;
            uint32_t nb_dst;
            piece_addr(NS - 1, b + NS - 1, nb_src, nb_dst);
            // A fragments on v_mfma_i32_16x16x64_i8: q4[2 rh + ks] = row (lane & 15) + 16 rh, bytes 64 ks + 16 (lane >> 4) ..+15
            // (quad 4 ks + (lane >> 4)); rows 16 apart share a rotation, so the second row half is the first + 2 KiB
            const char* slot = lds_ptr + (b % NS) * kPieceBytes + r16 * 128;
            f32x4 q4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                q4[j] = *reinterpret_cast<const f32x4*>(slot + (((4 * (j & 1) + g16) * 16 - rot16) & 112) + 2048 * (j >> 1));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < ND; ++n)
                dma_one(nb_src, nb_dst + n * 1024, voff[n], q4[n].x);
            const uint32_t cur_phys = phys[0];
#pragma unroll
            for (int j = 0; j < D; ++j) phys[j] = phys[j + 1];
            phys[D] = next_phys();
            const uint32_t row0 = cur_phys * kPieceRows;
#pragma unroll
            for (int half = 0; half < QH; ++half) {
                // 8 query blocks of 16 x 2 row halves: acc[rh][c][e] = row 16 rh + 4 (lane >> 4) + e, query 16 (8 half + c) + (lane & 15)
                constexpr int NC = 2 * NQB;
                i32x4 acc[2][NC];
                int thr16[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) thr16[c] = thr_lds[(half * NC + c) * 16 + r16];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    // all 16 accumulators per k-step (an accumulator's second MFMA never waits for its first); a query block's two
                    // row halves finish together, so its test starts under the MFMAs that remain
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int rh = 0; rh < 2; ++rh) {
                            constexpr int kLdsFrag = NQT * KS - 2;      // (flat B fragment (16-query block, k-step); the last two: LDS)
                            const int f = (half * NC + c) * 2 + ks;
                            uint4 bq;
                            if (f >= kLdsFrag) bq = *reinterpret_cast<const uint4*>(b_lds + (f - kLdsFrag) * 1024 + lane * 16);
                            else bq = bfrag[f / KS][f % KS];
                            const i32x4 c0 = ks == 0 ? i32x4{0, 0, 0, 0} : acc[rh][c];
                            acc[rh][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, q4[2 * rh + ks]),
                                                                               __builtin_bit_cast(i32x4, bq), c0, 0, 0, 0);
                        }
                    if (ks == 0) __builtin_amdgcn_sched_barrier(0);
                }
                uint64_t cmask[NC];
                bool hit[NC];
                uint64_t any_mask = 0;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    // the lane's eight values of a column block belong to ONE query
                    int m = acc[0][c][0];
#pragma unroll
                    for (int r = 1; r < 8; ++r) m = acc[r >> 2][c][r & 3] > m ? acc[r >> 2][c][r & 3] : m;
                    hit[c] = m >= thr16[c];
                    cmask[c] = __builtin_amdgcn_ballot_w64(hit[c]);
                    any_mask |= cmask[c];
                }
                if (any_mask != 0) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (cmask[c] == 0) continue;
                        uint64_t pend = cmask[c];
                        bool mine = hit[c];
                        for (;;) {
                            const uint32_t n = (uint32_t)__popcll(pend);
                            if (rec_st + n > kRecStage && rec_st != 0) rec_flush();
                            const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(pend >> 32),
                                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)pend, 0u));
                            const bool take = mine && pre < kRecStage;      // (more than kRecStage hit lanes: in rounds)
                            if (take) {
                                char* const r = rec_lds + (rec_st + pre) * kRecBytes;
                                *reinterpret_cast<i32x4*>(r) = acc[0][c];
                                *reinterpret_cast<i32x4*>(r + 16) = acc[1][c];
                                // (opaque: else the 16 tags of a lane are hoisted and live — spilled — across the block loop)
                                uint32_t tag = tag16;
                                asm volatile("" : "+v"(tag));
                                *reinterpret_cast<uint2*>(r + 32) = make_uint2(row0, tag + (uint32_t)((half * NC + c) * 16));
                            }
                            rec_st += n < kRecStage ? n : kRecStage;
                            if (n <= kRecStage) break;
                            mine = mine && !take;
                            pend = __builtin_amdgcn_ballot_w64(mine);
                        }
                    }
                }
            }
        }
        rec_flush();
        if (lane == 0) a.rec_cnt[gw] = rec_total;
    } else {
    for (uint32_t b = 0; b < nblk; ++b) {
        AccT acc[NQB];
#pragma unroll
        for (int c = 0; c < NQB; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0;
#pragma unroll
        for (int pc = 0; pc < PPB; ++pc) {
            const uint32_t t = b * PPB + pc;
            wait_vmcnt<ND * (NS - 2)>();
            const char* nb_src;
            uint32_t nb_dst;
            piece_addr(pc + NS - 1, t + NS - 1, nb_src, nb_dst);
            const char* slot = lds_ptr + (t % NS) * kPieceBytes + rd_row;
            // A fragment of k-step ksl (32 B of the row = quads 2ksl, 2ksl+1: 16 bf16 or 32 int8 columns): this
            // lane's half is quad 2ksl + h — one ds_read_b128 is one MFMA operand, no conversion
            f32x4 q4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int quad = 2 * j + h;
                q4[j] = *reinterpret_cast<const f32x4*>(slot + ((quad * 16 - rd_rot) & 112));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < ND; ++n)
                dma_one(nb_src, nb_dst + n * 1024, voff[n], q4[n].x);
#pragma unroll
            for (int ksl = 0; ksl < 4; ++ksl) {
                const bf16x8 af = __builtin_bit_cast(bf16x8, q4[ksl]);
                const int ks = pc * 4 + ksl;
#pragma unroll
                for (int c = 0; c < NQB; ++c) {
                    if constexpr (I8)
                        acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, q4[ksl]),
                                                                       __builtin_bit_cast(i32x4, bfrag[c][ks]), acc[c], 0, 0, 0);
                    else
                        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(bf16x8, bfrag[c][ks]), acc[c], 0, 0, 0);
                }
            }
        }
        const uint32_t cur_phys = phys[0];
#pragma unroll
        for (int j = 0; j < D; ++j) phys[j] = phys[j + 1];
        phys[D] = next_phys();
        // ---- screen test.  Each lane packs its hits into a bit set (bit c*16+r ↔ accumulator c,
        // register r); the slow path below only needs (row, query) — both follow from the bit index —
        // so the accumulators are never indexed dynamically.
        // Block reject: the largest of a lane's 16 bounds per query block against the screen threshold
        // (7 max3 + 1 max + 1 compare per query block).  fmaxf drops a NaN operand, which is safe: the
        // accumulators of a finite table and a finite, moderate query are finite, and every other query
        // has thr_screen = -inf (screen_thr_kernel) so that everything passes.  Inactive query columns
        // carry thr_s = +inf (and eps_unit 0).
        // bf16: this block's cutoffs, cut = thr - eps_unit x (largest row norm of the block), rounded down (the margin
        // term is kept finite so that +-inf thresholds stay what they are)
        ThrT cut[NQB];
        float nxr[16];                                   // L2 = 2: |x|^2 of this lane's 16 rows of the block
        if constexpr (L2 == 2) {
            const float* const nxp = a.nx_rows + (size_t)cur_phys * kPieceRows;      // wave-uniform: scalar loads
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                const float nxa = nxp[ro], nxb = nxp[ro + 4];
                nxr[r] = h ? nxb : nxa;
            }
#pragma unroll
            for (int c = 0; c < NQB; ++c) cut[c] = 0;
        } else if constexpr (L2 == 1) {
            // the block's integer cutoffs: floor(A_q + B_q * (smallest |x|^2 of the block)) - 2 (rounded down twice over;
            // -inf / NaN / below the int range: everything is a suspect)
            const float nxm = a.blk_nxmin[cur_phys];
#pragma unroll
            for (int c = 0; c < NQB; ++c) {
                const float v = __fmaf_rn(eu[c], nxm, la[c]);
                // (-inf or NaN: everything is a suspect; +inf — an inactive query column — or beyond the int range: nothing is)
                cut[c] = !(v > -2.0e9f) ? (int)0x80000000
                                        : (v >= 2.0e9f ? 0x7fffffff : __float2int_rd(v - fabsf(v) * 2.4e-7f - 2.0f));
            }
        } else if constexpr (I8) {
#pragma unroll
            for (int c = 0; c < NQB; ++c) cut[c] = thr_s[c];
        } else {
            // (the floor: a block of rows whose fp32 squares underflow reports a norm of zero, and components below 2^-126 keep an
            //  absolute 2^-134 in bf16, not a relative 2^-9 — such a block gets the margin of a row of norm kScreenNormFloor)
            const float nb = fmaxf(sqrtf(a.blk_norm2[cur_phys]), kScreenNormFloor) * 1.0002f;
#pragma unroll
            for (int c = 0; c < NQB; ++c) {
                const float v = __fmaf_rn(-eu[c], nb, thr_s[c]);
                cut[c] = v - __fmaf_rn(fminf(fabsf(v), 3.0e38f), 1.2e-7f, 1e-37f);
            }
        }
        uint64_t cmask[NQB];
        uint64_t any_mask = 0;
#pragma unroll
        for (int c = 0; c < NQB; ++c) {
            if constexpr (L2 == 2) {
                // per-ROW test: 2 s_x s_q I - |x|^2 against C'_q, in fp32 (|I| < 2^24 converts exactly; the roundings are in C'_q)
                float m = -__builtin_inff();
#pragma unroll
                for (int r = 0; r < 16; ++r) m = fmaxf(m, __fmaf_rn((float)acc[c][r], eu[c], -nxr[r]));
                cmask[c] = __builtin_amdgcn_ballot_w64(!(m < la[c]));
            } else if constexpr (I8) {
                int m = acc[c][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) m = acc[c][r] > m ? acc[c][r] : m;
                cmask[c] = __builtin_amdgcn_ballot_w64(m >= cut[c]);
            } else {
                float m = acc[c][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[c][r]);
                cmask[c] = __builtin_amdgcn_ballot_w64(!(m < cut[c]));
            }
            any_mask |= cmask[c];
        }
        if (any_mask != 0) {
            // the rare block with a hit: only the query blocks that have one are looked at again
            const uint32_t row0 = cur_phys * kPieceRows;
#pragma unroll
            for (int c = 0; c < NQB; ++c) {
                if (cmask[c] == 0) continue;
                // per-lane bit set of this query block: bit 15 - r ↔ register r (the compare sets VCC,
                // add-with-carry shifts it in: m = 2m + pass).  The accumulators were all read by the max
                // chains above, so the MFMA → VALU hazard the compiler cannot see inside asm is covered.
                uint32_t m16 = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (L2 == 2) {
                        const float g = __fmaf_rn((float)acc[c][r], eu[c], -nxr[r]);
                        asm volatile("v_cmp_nlt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                                     : "+v"(m16) : "v"(g), "v"(la[c]) : "vcc");
                    } else if constexpr (I8)
                        asm volatile("v_cmp_ge_i32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                                     : "+v"(m16) : "v"(acc[c][r]), "v"(cut[c]) : "vcc");
                    else
                        asm volatile("v_cmp_nlt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                                     : "+v"(m16) : "v"(acc[c][r]), "v"(cut[c]) : "vcc");
                }
                if (row0 + kPieceRows > a.row_end) {        // last block of a ragged table: drop rows past the end
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (row0 + (r & 3) + 8 * (r >> 2) + 4 * h >= a.row_end) m16 &= ~(1u << (15 - r));
                }
                // stage the hits, one per lane per round (ballot + prefix count: no LDS atomics, no waits)
                for (;;) {
                    const bool p = m16 != 0;
                    const uint64_t bm = __builtin_amdgcn_ballot_w64(p);
                    if (bm == 0) break;
                    const uint32_t n = __popcll(bm);
                    if (st_n + n > (uint32_t)kCap) flush();
                    if (p) {
                        const int r = 15 - __builtin_ctz(m16);
                        const uint32_t pos = st_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32),
                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
                        st_row[pos] = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        st_q[pos] = (uint32_t)(c * 32 + i32);
                        m16 &= m16 - 1;
                    }
                    st_n += n;
                }
            }
        }
    }
    }
    if constexpr (QH == 1) flush();
    wait_vmcnt<0>();
}

// hit records → per-query suspect lists (see kRecBytes).  One workgroup per scan workgroup (its eight wave regions), one
// record per thread and round.  Two passes over the records: count per query in LDS, ONE global atomic per query and
// workgroup to reserve the range (one per suspect — 2.3 M returning atomics on 256 counters — made this kernel take 1.08 ms),
// then place the rows.
__device__ __forceinline__ uint32_t rec_mask(const char* r, const float* __restrict__ thr_screen, uint32_t row_end, uint32_t& q,
                                             uint32_t& row0h) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    // D of v_mfma_i32_16x16x64_i8: lane l holds column l & 15 (the query), rows 4 (l >> 4) + e in register e = 0..3; the record
    // is the lane's two row halves (registers rr = 0..3: rows 0-15 of the block, rr = 4..7: rows 16-31) and the tag
    // (block's first row; query | (l >> 4) << 8)
    const uint2 tag = *reinterpret_cast<const uint2*>(r + 32);
    q = tag.y & 255u;
    const uint32_t g = (tag.y >> 8) & 3u;
    row0h = tag.x + 4 * g;
    const int t = __float_as_int(thr_screen[q]);
    uint32_t m = 0;                                        // bit rr: accumulator register rr of the lane is a suspect
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const i32x4 v = *reinterpret_cast<const i32x4*>(r + 16 * jj);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rr = 4 * jj + e;
            if (v[e] >= t && row0h + (rr & 3) + 16 * (rr >> 2) < row_end) m |= 1u << rr;
        }
    }
    return m;
}
__global__ __launch_bounds__(1024) void screen_decode_kernel(const char* __restrict__ rec, const uint32_t* __restrict__ rec_cnt,
                                                             uint32_t rec_cap, uint32_t rec_waves, const char* __restrict__ rec_pool,
                                                             uint32_t rec_pool_cap, const float* __restrict__ thr_screen, uint32_t row_end,
                                                             uint32_t* __restrict__ susp_cnt, uint32_t* __restrict__ susp,
                                                             uint32_t cap, uint32_t* __restrict__ overflow) {
    __shared__ uint32_t cntq[kMaxQueries], baseq[kMaxQueries], nreg[8];
    // pass 1 leaves (first row + 4 x lane group, query | mask << 16) of every record with a suspect here, pass 2 reads them back
    // (records beyond the buffer — a workgroup of a skewed table — are read from global memory again)
    constexpr uint32_t kKeep = 12288;
    __shared__ uint2 keep[kKeep];
    // workgroups [0, rec_waves / 8): the eight wave regions of one scan workgroup; the ones behind: a slice of the spill pool
    const bool pool = blockIdx.x >= rec_waves / 8;
    if (threadIdx.x < kMaxQueries) cntq[threadIdx.x] = 0;
    if (threadIdx.x < 8) {
        uint32_t n;
        if (pool) {
            const uint32_t filled = rec_cnt[rec_waves] < rec_pool_cap ? rec_cnt[rec_waves] : rec_pool_cap;
            const uint32_t begin = (blockIdx.x - rec_waves / 8) * kRecPoolSlice;
            n = threadIdx.x == 0 && begin < filled ? (filled - begin < kRecPoolSlice ? filled - begin : kRecPoolSlice) : 0u;
        } else {
            const uint32_t n_raw = rec_cnt[blockIdx.x * 8 + threadIdx.x];
            n = n_raw < rec_cap ? n_raw : rec_cap;
        }
        nreg[threadIdx.x] = n;
    }
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t off = 0;
        for (uint32_t w = 0; w < 8; ++w) {
            const uint32_t n = nreg[w];
            const char* const base = pool ? rec_pool + (size_t)(blockIdx.x - rec_waves / 8) * kRecPoolSlice * kRecBytes
                                          : rec + (size_t)(blockIdx.x * 8 + w) * rec_cap * kRecBytes;
            for (uint32_t e = threadIdx.x; e < n; e += 1024) {
                uint32_t q, row0h, m;
                const uint32_t slot = off + e;
                if (pass == 1 && slot < kKeep) {
                    const uint2 kp = keep[slot];
                    row0h = kp.x;
                    q = kp.y & 0xffffu;
                    m = kp.y >> 16;
                } else {
                    m = rec_mask(base + (size_t)e * kRecBytes, thr_screen, row_end, q, row0h);
                    if (pass == 0 && slot < kKeep) keep[slot] = make_uint2(row0h, q | (m << 16));
                }
                if (m == 0) continue;
                const uint32_t nh = __popc(m);
                if (pass == 0) {
                    atomicAdd(&cntq[q], nh);
                } else {
                    uint32_t pos = baseq[q] + atomicAdd(&cntq[q], nh);
                    if (pos + nh > cap) { *overflow = 1u; continue; }
                    while (m) {
                        const uint32_t rr = __builtin_ctz(m);
                        m &= m - 1;
                        susp[(uint64_t)q * cap + pos++] = row0h + (rr & 3) + 16 * (rr >> 2);
                    }
                }
            }
            off += n;
        }
        __syncthreads();
        if (pass == 0 && threadIdx.x < kMaxQueries) {
            const uint32_t c = cntq[threadIdx.x];
            baseq[threadIdx.x] = c ? atomicAdd(&susp_cnt[threadIdx.x], c) : 0u;
            cntq[threadIdx.x] = 0;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// rescore: exact scores of the suspects a screened launch parked in susp[q][0..susp_cnt[q]) — the
// specification's k-ascending fmaf chain over the fp32 table row and the fp32 query — keeping those
// with !(s < thr[q]) as candidate keys in cand[q].  One block = 256 suspects of ONE query (grid.y = query,
// grid.x strides over the list): the query sits in LDS (broadcast reads), each wave gathers its 64 rows
// with coalesced 256 B segments into a padded LDS tile (16 independent loads per lane in flight), then
// lane s walks row s.  One returning atomic per block reserves the output range.
// rescore_kernel's two steps on one unit (a 256-B half of 64 rows): the gather of the wave's 64 rows (16
// independent 16-B loads per lane, four rows per instruction) and the walk (LDS tile, then lane s runs the
// specification's k-ascending fmaf chain over row s)
template <int DIM>
__device__ __forceinline__ void rescore_gather(f32x4 (&buf)[16], const float* __restrict__ tab, uint32_t row, int ph, int lane) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t r_i = (uint32_t)__shfl((int)row, 4 * i + (lane >> 4), 64);
        buf[i] = reinterpret_cast<const f32x4*>(tab + (size_t)r_i * DIM + ph * 64)[lane & 15];
    }
}
template <int ROWB>
__device__ __forceinline__ void rescore_walk(const f32x4 (&buf)[16], char* my, const float* qs, int ph, int lane, float& s) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
        *reinterpret_cast<f32x4*>(my + (4 * i + (lane >> 4)) * ROWB + (lane & 15) * 16) = buf[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float4 x = *reinterpret_cast<const float4*>(my + lane * ROWB + k * 16);
        const float4 y = *reinterpret_cast<const float4*>(&qs[ph * 64 + 4 * k]);
        s = __fmaf_rn(x.x, y.x, s);
        s = __fmaf_rn(x.y, y.y, s);
        s = __fmaf_rn(x.z, y.z, s);
        s = __fmaf_rn(x.w, y.w, s);
        // (keeps hipcc from hoisting all 32 LDS reads above the chain: with two gathers in flight that pushed the
        // kernel past 256 registers and one gather buffer into scratch)
        if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_wave_barrier();
}

// (L2: the exact inner product is turned into -d = fmaf(2, ip, -(|x|^2 + |q|^2)) before the threshold test and the key)
template <int DIM, bool L2 = false>
__global__ __launch_bounds__(256) void rescore_kernel(const float* __restrict__ tab, const float* __restrict__ qpad,
                                                      const float* __restrict__ thr,
                                                      const uint32_t* __restrict__ susp,
                                                      const uint32_t* __restrict__ susp_cnt, uint32_t cap,
                                                      uint32_t* __restrict__ cnt, uint64_t* __restrict__ cand,
                                                      uint32_t* __restrict__ overflow, uint32_t scap, uint32_t n_rows,
                                                      const float* __restrict__ nx = nullptr, const float* __restrict__ nqv = nullptr,
                                                      RowFilter filter = RowFilter()) {
    // (scap: capacity and stride of the suspect lists; cap: of the candidate lists)
    constexpr int kRowB = 64 * 4 + 16;                 // 64 columns per phase, padded: conflict-free b128 column walks
    __shared__ __attribute__((aligned(16))) char tile[4][64 * kRowB];
    __shared__ __attribute__((aligned(16))) float qs[DIM];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t base_s;
    const uint32_t q = blockIdx.y;
    const uint32_t n_raw = susp_cnt[q];
    const uint32_t n = n_raw < scap ? n_raw : scap;
    if (blockIdx.x * 256u >= n) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < DIM) qs[threadIdx.x] = qpad[(size_t)q * DIM + threadIdx.x];
    const float thr_q = thr[q];
    __syncthreads();
    char* const my = tile[w];
    // The gathers run one unit (a 256-B half of 64 rows) ahead of the arithmetic: while a wave walks one half-row
    // tile, the loads of the next half — or of the next chunk's first half — are in flight (one exposed HBM round
    // trip per chunk and phase before).
    // (a list that overflowed has holes — the decode kernel reserves a run of slots and writes none of it when the run crosses
    //  the capacity — whose stale contents may be rows of an earlier, larger table: the plan is discarded, but the gather must
    //  stay inside this table.  Found as a memory fault by scripts/soak_adversarial.py: zero queries, every row a tie.)
    auto row_of = [&](uint32_t t0) -> uint32_t {
        const uint32_t e = t0 + threadIdx.x;
        const uint32_t r = e < n ? susp[(uint64_t)q * scap + e] : 0u;
        return r < n_rows ? r : 0u;
    };
    constexpr int NPH = DIM / 64;
    const uint32_t step = gridDim.x * 256u;
    uint32_t t0 = blockIdx.x * 256u;
    uint32_t row = row_of(t0);
    f32x4 va[16], vb[16];              // (ext vectors: HIP's float4 struct made these loop-carried buffers memcpy'd stack objects)
    rescore_gather<DIM>(va, tab, row, 0, lane);
    for (; t0 < n; t0 += step) {
        const bool valid = t0 + threadIdx.x < n;
        const uint32_t row_next = t0 + step < n ? row_of(t0 + step) : 0u;
        float s = 0.0f;
        // (phases written out: with `v[ph & 1]` inside a loop the buffers stayed in scratch at DIM = 128; past the
        // last chunk row_next is 0 — a harmless gather of row 0 instead of a conditional one)
        // (every phase is walked in column order: the chain is k-ascending over all DIM columns)
        if constexpr (NPH == 1) {
            rescore_gather<DIM>(vb, tab, row_next, 0, lane);
            rescore_walk<kRowB>(va, my, qs, 0, lane, s);
        } else if constexpr (NPH == 2) {
            rescore_gather<DIM>(vb, tab, row, 1, lane);
            rescore_walk<kRowB>(va, my, qs, 0, lane, s);
            rescore_gather<DIM>(va, tab, row_next, 0, lane);
            rescore_walk<kRowB>(vb, my, qs, 1, lane, s);
        } else if constexpr (NPH == 3) {
            rescore_gather<DIM>(vb, tab, row, 1, lane);
            rescore_walk<kRowB>(va, my, qs, 0, lane, s);
            rescore_gather<DIM>(va, tab, row, 2, lane);
            rescore_walk<kRowB>(vb, my, qs, 1, lane, s);
            rescore_gather<DIM>(vb, tab, row_next, 0, lane);
            rescore_walk<kRowB>(va, my, qs, 2, lane, s);
        } else {
            static_assert(NPH == 4, "rescore_kernel: DIM 64, 128, 192 or 256");
            rescore_gather<DIM>(vb, tab, row, 1, lane);
            rescore_walk<kRowB>(va, my, qs, 0, lane, s);
            rescore_gather<DIM>(va, tab, row, 2, lane);
            rescore_walk<kRowB>(vb, my, qs, 1, lane, s);
            rescore_gather<DIM>(vb, tab, row, 3, lane);
            rescore_walk<kRowB>(va, my, qs, 2, lane, s);
            rescore_gather<DIM>(va, tab, row_next, 0, lane);
            rescore_walk<kRowB>(vb, my, qs, 3, lane, s);
        }
        if (NPH & 1) {                                   // odd phase count: the prefetched unit sits in v[1], the loop reads v[0]
#pragma unroll
            for (int i = 0; i < 16; ++i) va[i] = vb[i];
        }
        if constexpr (L2) s = __fmaf_rn(2.0f, s, -(nx[row] + nqv[q]));
        const bool keep = valid && !(s < thr_q) && row_filter_pass(filter, row);
        const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            base_s = tot ? atomicAdd(&cnt[q], tot) : 0u;
        }
        __syncthreads();
        uint32_t pos = base_s + before;
        for (int j = 0; j < w; ++j) pos += wsum[j];
        if (keep) {
            if (pos < cap) cand[(uint64_t)q * cap + pos] = topk_key(s, row);
            else *overflow = 1u;
        }
        __syncthreads();
        row = row_next;
    }
    if (n_raw > scap && threadIdx.x == 0) *overflow = 1u;
}

// per call: bf16 B fragments of the (zero-padded) queries and eps_unit_q = kScreenEps * ||q|| (the screen multiplies it
// by the largest row norm of each 32-row block: the bf16 bound is relative to the row, so one huge row does not
// loosen it for the rest of the table)
__global__ void screen_prep_kernel(const float* __restrict__ qpad, uint32_t dim,
                                   uint4* __restrict__ qb16, float* __restrict__ eps) {
    const uint32_t KS = dim / 16;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint32_t)kScreenMaxNQB * KS * 64) {
        const uint32_t lane = i & 63, ks = (i >> 6) % KS, c = (i >> 6) / KS;
        const float* q = qpad + (size_t)(c * 32 + (lane & 31)) * dim + ks * 16 + 8 * (lane >> 5);
        uint32_t w[4];
        for (int e = 0; e < 4; ++e) {
            auto rne = [](float x) -> uint32_t {
                uint32_t b = __float_as_uint(x);
                if ((b & 0x7FFFFFFFu) > 0x7F800000u) return (b >> 16) | 0x40u;
                b += 0x7FFFu + ((b >> 16) & 1u);
                return b >> 16;
            };
            w[e] = rne(q[2 * e]) | (rne(q[2 * e + 1]) << 16);
        }
        qb16[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (i < (uint32_t)kMaxQueries) {
        double ss = 0.0;
        for (uint32_t k = 0; k < dim; ++k) {
            const double v = (double)qpad[(size_t)i * dim + k];
            ss += v * v;
        }
        // inflated so that it is an upper bound in fp32
        eps[i] = (float)(sqrt(ss) * (double)kScreenEps * 1.0001) + 1e-30f;
    }
}

// bf16 screen: thr_screen = thr (the margin is applied per block in the kernel), or -inf
__global__ void screen_thr_kernel(const float* __restrict__ thr, const float* __restrict__ eps, float max_norm,
                                  float* __restrict__ thr_screen) {
    const uint32_t q = threadIdx.x;
    if (q >= (uint32_t)kMaxQueries) return;
    const float t = thr[q], e = eps[q];
    // the kernel subtracts eps_unit x block norm itself; non-finite queries, or magnitudes whose bf16 partial sums
    // could overflow — |partial sum| <= ||x|| ||q|| = 125 eps_unit ||x||, and an inf - inf accumulator would be a NaN
    // that the block-reject max chain drops silently — : everything passes the screen and the exact re-scoring decides
    float v = t;
    if (!(e == e) || e > 1e28f || !(t == t) || !(e * max_norm < 1e35f)) v = -__builtin_inff();
    thr_screen[q] = v;
}

// ---- int8 screen (dim 128).  x^ = s_x X, q^ = s_q Q with X, Q in [-127, 127]; the MFMA gives the integer dot
// product I = sum X_i Q_i exactly.  For the true score s = sum x_i q_i (real arithmetic):
//     s - s_x s_q I = sum (x_i - x^_i) q_i + sum x^_i (q_i - q^_i)
//     |s - s_x s_q I| <= ||x - x^|| ||q|| + ||x^|| ||q - q^||  <=  R ||q|| + (N + R) ||q - q^||
// with R = max row residual (TableDerived::resid8, measured when the shadow is built), N = max row norm.  eps_q is
// that bound plus 1e-5 N ||q|| for the rounding of the specification's fp32 fmaf chain (<= 128 * 2^-24 N ||q||).
// A row can reach thr only if  I >= (thr - eps_q) / (s_x s_q): the screen compares integers.
// per call: int8 B fragments of the (zero-padded) queries, eps_q and the per-query scale s_q = max|q| / 127
// One workgroup per query block of 32 in use (the other slots of the 256 are neither read by the scan nor prepared:
// a single request used to spend 36 us preparing 255 zero queries, a full batch 37 us in one 1024-thread workgroup).
__global__ __launch_bounds__(128) void screen_prep8_kernel(const float* __restrict__ qpad, uint32_t dim,
                                                            float max_norm, float resid, uint4* __restrict__ qb8,
                                                            float* __restrict__ eps, float* __restrict__ qscale, uint32_t wide) {
    __shared__ float sq[32];
    const uint32_t tid = threadIdx.x, c = blockIdx.x;
    {
        // four threads per query, a quarter of the columns each
        const uint32_t ql = tid >> 2, qi = c * 32 + ql, part = tid & 3, per = dim / 4;
        const float* q = qpad + (size_t)qi * dim + part * per;
        float mx = 0.0f;
        bool bad = false;
        for (uint32_t k = 0; k < per; ++k) {
            const float v = fabsf(q[k]);
            if (!(v <= 3.0e38f)) bad = true;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        bad = (__shfl_xor((int)bad, 1, 64) | (int)bad) != 0;
        bad = (__shfl_xor((int)bad, 2, 64) | (int)bad) != 0;
        const float sc = fmaxf(mx / 127.0f, 1e-30f);
        double ss = 0.0, dd = 0.0;
        for (uint32_t k = 0; k < per; ++k) {
            const double v = (double)q[k];
            int Q = __float2int_rn(q[k] / sc);
            Q = Q > 127 ? 127 : (Q < -127 ? -127 : Q);
            const double d = v - (double)sc * (double)Q;
            ss += v * v;
            dd += d * d;
        }
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        dd += __shfl_xor(dd, 1, 64);
        dd += __shfl_xor(dd, 2, 64);
        if (part == 0) {
            // (sums of non-negative terms: any summation order is an upper bound once inflated below)
            const double nq = sqrt(ss), dq = sqrt(dd);
            const double e = ((double)resid * nq + ((double)max_norm + (double)resid) * dq) * 1.0001 +
                             1e-5 * (double)max_norm * nq + 1e-30;
            eps[qi] = bad ? __builtin_nanf("") : (float)(e * 1.000001);      // upper bound in fp32
            qscale[qi] = sc;
            sq[ql] = sc;
        }
    }
    __syncthreads();
    // B fragments, 16 B per lane.  v_mfma_i32_32x32x32_i8: [c][ks][lane] = query 32 c + (lane & 31), bytes 32 ks + 16 (lane >> 5) ..+15.
    // wide (> 128 queries, dim 128: the query halves run on v_mfma_i32_16x16x64_i8): [c16][ks][lane] = query 16 c16 + (lane & 15),
    // bytes 64 ks + 16 (lane >> 4) ..+15, two k-steps — this workgroup's 32 queries are blocks c16 = 2 c, 2 c + 1, the same 4 x 64 slots
    const uint32_t KS = dim / 32;
    for (uint32_t i = tid; i < KS * 64; i += blockDim.x) {
        const uint32_t lane = i & 63, ks = wide ? (i >> 6) & 1 : i >> 6;
        const uint32_t ql = wide ? 16 * (i >> 7) + (lane & 15) : lane & 31;
        const float* q = qpad + (size_t)(c * 32 + ql) * dim + (wide ? ks * 64 + 16 * (lane >> 4) : ks * 32 + 16 * (lane >> 5));
        const float sc = sq[ql];
        uint32_t w[4];
        for (int e = 0; e < 4; ++e) {
            uint32_t word = 0;
            for (int b = 0; b < 4; ++b) {
                int Q = __float2int_rn(q[4 * e + b] / sc);
                Q = Q > 127 ? 127 : (Q < -127 ? -127 : Q);
                word |= (uint32_t)(Q & 0xff) << (8 * b);
            }
            w[e] = word;
        }
        qb8[c * KS * 64 + i] = make_uint4(w[0], w[1], w[2], w[3]);      // (= [c][ks][lane], wide: [2 c + (i >> 7)][ks][lane])
    }
}

// integer screen threshold: T = floor((thr - eps) / (s_x s_q)) - 1 as int32 bits (INT_MIN: everything passes)
__global__ void screen_thr8_kernel(const float* __restrict__ thr, const float* __restrict__ eps,
                                   const float* __restrict__ qscale, float s_x, float* __restrict__ thr_screen) {
    const uint32_t q = threadIdx.x;
    if (q >= (uint32_t)kMaxQueries) return;
    const float t = thr[q], e = eps[q];
    int T = (int)0x80000000;
    if (e == e && e <= 1e30f && t == t && t > -__builtin_inff()) {
        const double v = floor(((double)t - (double)e) / ((double)s_x * (double)qscale[q])) - 1.0;
        T = v >= 2147483647.0 ? 0x7fffffff : (v <= -2147483648.0 ? (int)0x80000000 : (int)v);
    }
    thr_screen[q] = __int_as_float(T);
}

// Squared-Euclidean recall on the int8 screen.  A pair can reach the threshold thr (in -d units) only if, in exact arithmetic,
// 2 ip - |x|^2 - |q|^2 >= thr - delta (delta: the rounding of the specification's own fp32 evaluation of -d), i.e.
// ip >= (thr - delta + |q|^2) / 2 + |x|^2 / 2; with ip <= s_x s_q I + eps_q (the inner-product screen's bound) and |x|^2 >= the
// block's smallest: I >= A_q + B_q min|x|^2,  A_q = ((thr - delta + |q|^2) / 2 - eps_q) / (s_x s_q),  B_q = 1 / (2 s_x s_q).
// Both are rounded down here, the kernel rounds the sum down again.  thr = -inf (or anything odd): A_q = -inf, everything passes.
__global__ void screen_thr8_l2_kernel(const float* __restrict__ thr, const float* __restrict__ eps, const float* __restrict__ qscale,
                                      const float* __restrict__ nqv, float s_x, float max_norm, float* __restrict__ a_out,
                                      float* __restrict__ b_out, int per_row) {
    const uint32_t q = threadIdx.x;
    if (q >= (uint32_t)kMaxQueries) return;
    const float t = thr[q], e = eps[q];
    const double nq = (double)nqv[q], N = (double)max_norm;
    const double sq = (double)s_x * (double)qscale[q];
    float A = -__builtin_inff(), B = 0.0f;
    if (e == e && e <= 1e30f && t == t && t > -__builtin_inff() && sq > 0.0 && nq == nq && nq < 1e30) {
        const double delta = 2e-6 * (N * N + nq + 2.0 * N * sqrt(nq)) + 1e-30;
        if (per_row) {
            // per-row form: 2 s_x s_q I - |x|^2 >= thr - delta + |q|^2 - 2 eps_q =: C_q, evaluated by the kernel as
            // fmaf((float)I, c1, -|x|^2) with c1 = 2 s_x s_q rounded UP (I can be negative: the product's error is covered
            // with the fma's by a second delta)
            const double c = (double)t - 2.0 * delta + nq - 2.0 * (double)e;
            A = (float)(c - fabs(c) * 1e-6 - 1e-30);
            B = (float)(2.0 * sq);
            if (!(A == A) || !(B == B) || B > 1e30f) { A = -__builtin_inff(); B = 0.0f; }
        } else {
            const double a = (((double)t - delta + nq) * 0.5 - (double)e) / sq;
            const double b = 0.5 / sq;
            A = (float)(a - fabs(a) * 1e-6 - 1.0);
            B = (float)(b * (1.0 - 1e-6));
            if (!(A == A) || !(B == B) || B > 1e30f) { A = -__builtin_inff(); B = 0.0f; }
        }
    }
    a_out[q] = A;
    b_out[q] = B;
}


// squared-Euclidean recall: |q|^2 of every query as a k-ascending fmaf chain (the specification's; |x|^2 of every row:
// recall_table.hip), and the sign flip of the scores that come out (-d → d; padding -inf → +inf)
__global__ void query_norm2_kernel(const float* __restrict__ qpad, uint32_t dim, float* __restrict__ out) {
    const uint32_t q = threadIdx.x;
    float s = 0.0f;
    for (uint32_t c = 0; c < dim; ++c) s = __fmaf_rn(qpad[(size_t)q * dim + c], qpad[(size_t)q * dim + c], s);
    out[q] = s;
}
__global__ void negate_kernel(float* __restrict__ v, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = 0.0f - v[i];                     // (a zero distance comes out as +0, padding as +inf)
}

template <int DIM, int NQB = 1, bool L2 = false>
static int launch_scan(pg_ctx* ctx, const ScanArgs& a) {
    int rc_attr;
    if ((rc_attr = ensure_dyn_lds(ctx, (const void*)scan_kernel<DIM, NQB, 0, L2>, kScanLds))) return rc_attr;
    const uint32_t total = a.rb_end - a.rb_begin;
    uint32_t grid = (uint32_t)ctx->num_cus;
    const uint32_t need = (total + kScanWaves - 1) / kScanWaves;
    if (grid > need) grid = need;
    const uint32_t groups = a.group_q ? (a.nq + a.group_q - 1) / a.group_q : 1;
    scan_kernel<DIM, NQB, 0, L2><<<dim3(grid, groups), 64 * kScanWaves, kScanLds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int dispatch_scan(pg_ctx* ctx, uint32_t dim, const ScanArgs& a) {
    const bool wide = a.nq_launch > 32;          // two 32-query column blocks
    if (a.nx) {                                   // squared-Euclidean recall
        if (dim == 64) return wide ? launch_scan<64, 2, true>(ctx, a) : launch_scan<64, 1, true>(ctx, a);
        if (dim == 128) return wide ? launch_scan<128, 2, true>(ctx, a) : launch_scan<128, 1, true>(ctx, a);
        set_error("recall (squared Euclidean): dim=%u unsupported (64 or 128)", dim);
        return PG_ERR_UNSUPPORTED;
    }
    switch (dim) {
        case 64: return wide ? launch_scan<64, 2>(ctx, a) : launch_scan<64, 1>(ctx, a);
        case 128: return wide ? launch_scan<128, 2>(ctx, a) : launch_scan<128, 1>(ctx, a);
        case 192:
        case 256:
            if (wide) {      // 2 x dim/2 B-operand registers no longer fit 2 waves per SIMD
                set_error("recall: dim=%u supports at most 32 queries per pass (64 up to dim 128)", dim);
                return PG_ERR_UNSUPPORTED;
            }
            return dim == 192 ? launch_scan<192, 1>(ctx, a) : launch_scan<256, 1>(ctx, a);
    }
    set_error("recall: dim=%u unsupported", dim);
    return PG_ERR_UNSUPPORTED;
}

template <int DIM, int NQB, int WAVES, bool I8 = false, int QH = 1, int L2 = 0>
static int launch_screen(pg_ctx* ctx, const ScreenArgs& a) {
    int rc_attr;
    if ((rc_attr = ensure_dyn_lds(ctx, (const void*)screen_kernel<DIM, NQB, WAVES, 1, 0, I8, QH, L2>, kScreenLds))) return rc_attr;
    const uint32_t total = a.rb_end - a.rb_begin;
    uint32_t grid = (uint32_t)ctx->num_cus;
    const uint32_t need = (total + WAVES - 1) / WAVES;
    if (grid > need) grid = need;
    screen_kernel<DIM, NQB, WAVES, 1, 0, I8, QH, L2><<<grid, 64 * WAVES, kScreenLds, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

static int dispatch_screen(pg_ctx* ctx, uint32_t dim, bool i8, const ScreenArgs& a) {
    const bool wide = a.nq > 128;
    if (a.nx_rows) {                                 // squared-Euclidean recall, per-row test (rows of mixed norms)
        if (a.nq <= 32) return launch_screen<128, 1, 8, true, 1, 2>(ctx, a);
        if (a.nq <= 64) return launch_screen<128, 2, 8, true, 1, 2>(ctx, a);
        return launch_screen<128, 4, 8, true, 1, 2>(ctx, a);
    }
    if (a.blk_nxmin) {                               // squared-Euclidean recall: int8 shadow, <= 128 queries (recall_job_prepare)
        if (a.nq <= 32) return launch_screen<128, 1, 8, true, 1, 1>(ctx, a);
        if (a.nq <= 64) return launch_screen<128, 2, 8, true, 1, 1>(ctx, a);
        return launch_screen<128, 4, 8, true, 1, 1>(ctx, a);
    }
    if (i8) {                                        // int8 shadow (dim 128)
        if (wide) return launch_screen<128, 4, 8, true, 2>(ctx, a);
        if (a.nq <= 32) return launch_screen<128, 1, 8, true>(ctx, a);
        if (a.nq <= 64) return launch_screen<128, 2, 8, true>(ctx, a);
        return launch_screen<128, 4, 8, true>(ctx, a);
    }
    if (dim == 64) {
        if (wide) return launch_screen<64, 8, 4>(ctx, a);
        if (a.nq <= 32) return launch_screen<64, 1, 8>(ctx, a);
        if (a.nq <= 64) return launch_screen<64, 2, 8>(ctx, a);
        return launch_screen<64, 4, 8>(ctx, a);
    }
    if (wide) return launch_screen<128, 8, 4>(ctx, a);
    if (a.nq <= 32) return launch_screen<128, 1, 8>(ctx, a);
    if (a.nq <= 64) return launch_screen<128, 2, 8>(ctx, a);
    return launch_screen<128, 4, 8>(ctx, a);
}

int screen_launch(pg_ctx* ctx, uint32_t dim, bool i8, const ScreenArgs& a) {
    int rc;
    if ((rc = dispatch_screen(ctx, dim, i8, a))) return rc;
    if (a.rec) {
        screen_decode_kernel<<<a.rec_waves / 8 + a.rec_pool_cap / kRecPoolSlice, 1024, 0, ctx->stream>>>(
            a.rec, a.rec_cnt, a.rec_cap, a.rec_waves, a.rec_pool, a.rec_pool_cap, a.thr_screen, a.row_end, a.susp_cnt, a.susp, a.cap, a.overflow);
        PG_HIP(hipGetLastError());
    }
    return PG_OK;
}

int screen_prep_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, uint32_t nq, bool wide) {
    if (t->derived.shadow_is_i8)
        screen_prep8_kernel<<<nq <= 32 ? 1u : (nq <= 64 ? 2u : (nq <= 128 ? 4u : 8u)), 128, 0, ctx->stream>>>(
            rs.qpad, t->dim, t->derived.max_norm, t->derived.resid8, rs.qb16, rs.eps, rs.qscale,
            wide ? 1u : 0u);     // grid = the scan's NQB x QH; wide: dispatch_screen's query halves
    else
        screen_prep_kernel<<<(kScreenMaxNQB * (t->dim / 16) * 64 + 255) / 256, 256, 0, ctx->stream>>>(
            rs.qpad, t->dim, rs.qb16, rs.eps);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int screen_thr_launch(pg_ctx* ctx, const pg_table* t, const RecallScratch& rs, bool l2, bool l2_per_row) {
    if (l2) screen_thr8_l2_kernel<<<1, kMaxQueries, 0, ctx->stream>>>(rs.thr, rs.eps, rs.qscale, rs.pred_ms, t->derived.s8, t->derived.max_norm,
                                                                      rs.thr_screen, rs.thr_ref, l2_per_row ? 1 : 0);
    else if (t->derived.shadow_is_i8) screen_thr8_kernel<<<1, kMaxQueries, 0, ctx->stream>>>(rs.thr, rs.eps, rs.qscale, t->derived.s8, rs.thr_screen);
    else screen_thr_kernel<<<1, kMaxQueries, 0, ctx->stream>>>(rs.thr, rs.eps, t->derived.max_norm, rs.thr_screen);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// The exact re-scoring and the squared-Euclidean helpers, for the plans and for index_search.hip: the same kernels, so a
// row scored there carries the bits the table's own pass gives it.  blocks = 0: the table pass's own grid.
constexpr uint32_t kRescoreBlocksPerQuery = 16;   // x 256 suspects per block per stride step
int rescore_launch(pg_ctx* ctx, uint32_t dim, bool l2, const float* tab, const float* d_queries, const float* thr, const uint32_t* susp,
                   const uint32_t* susp_cnt, uint32_t scap, uint32_t* cnt, uint64_t* cand, uint32_t* overflow, uint32_t cap, uint32_t nq,
                   uint32_t n_rows, const float* nx, const float* nqv, uint32_t blocks, const RowFilter& filter) {
    const dim3 g(blocks ? blocks : kRescoreBlocksPerQuery, nq);
    if (l2 && dim == 64)
        rescore_kernel<64, true><<<g, 256, 0, ctx->stream>>>(tab, d_queries, thr, susp, susp_cnt, cap, cnt, cand, overflow, scap, n_rows, nx, nqv, filter);
    else if (l2 && dim == 128)
        rescore_kernel<128, true><<<g, 256, 0, ctx->stream>>>(tab, d_queries, thr, susp, susp_cnt, cap, cnt, cand, overflow, scap, n_rows, nx, nqv, filter);
    else if (!l2 && dim == 64)
        rescore_kernel<64><<<g, 256, 0, ctx->stream>>>(tab, d_queries, thr, susp, susp_cnt, cap, cnt, cand, overflow, scap, n_rows, nullptr, nullptr, filter);
    else if (!l2 && dim == 128)
        rescore_kernel<128><<<g, 256, 0, ctx->stream>>>(tab, d_queries, thr, susp, susp_cnt, cap, cnt, cand, overflow, scap, n_rows, nullptr, nullptr, filter);
    else if (!l2 && dim == 192)
        rescore_kernel<192><<<g, 256, 0, ctx->stream>>>(tab, d_queries, thr, susp, susp_cnt, cap, cnt, cand, overflow, scap, n_rows, nullptr, nullptr, filter);
    else if (!l2 && dim == 256)
        rescore_kernel<256><<<g, 256, 0, ctx->stream>>>(tab, d_queries, thr, susp, susp_cnt, cap, cnt, cand, overflow, scap, n_rows, nullptr, nullptr, filter);
    else {
        set_error("rescore: dim=%u unsupported%s", dim, l2 ? " (squared Euclidean: 64 or 128)" : "");
        return PG_ERR_UNSUPPORTED;
    }
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int query_norm2_launch(pg_ctx* ctx, const float* d_queries, uint32_t nq, uint32_t dim, float* d_out) {
    query_norm2_kernel<<<1, nq, 0, ctx->stream>>>(d_queries, dim, d_out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int negate_launch(pg_ctx* ctx, float* d_v, uint64_t n) {
    negate_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, ctx->stream>>>(d_v, n);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg
