// Microbenchmark: the 256-query int8 screen's block body on v_mfma_i32_32x32x32_i8 against v_mfma_i32_16x16x64_i8.
// Both kernels do, per wave and per block, what screen_kernel's query-half path does per 32-row table block:
// 32 rows x 256 queries x K = 128 in two query halves, the 128 B registers parked in the AGPR half, the four A fragments
// re-read from LDS with ds_read_b128 for every block (a rotated piece layout per shape, conflict-free: quad_off below),
// two waves per SIMD, one workgroup per CU, and the accumulators reduced with the screen's max / compare / ballot.
// Operands are random int8 over the full +-127 range (a constant or zero fill hides a clock difference between shapes), the
// thresholds sit at 3.7-4.2 sigma so a block has a hit lane about as often as the product's does.
// The two variants alternate in one process after ~2 s of back-to-back launches; wall time comes from events, cycles and the
// in-kernel clock from s_memtime / s_memrealtime stamps around the block loop.  Each hit also feeds a count and a
// (row, query) checksum, compared between the variants and against the host for workgroup 0: that checks both operand layouts
// and both output layouts.
// Build: hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form=1 -o mfma_shape_i8 mfma_shape_i8.hip
// Run:   mfma_shape_i8 [rounds=12] [launches per round=30] [blocks per wave=3000]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 8;            // two per SIMD
constexpr int kNS = 4;               // pieces per wave, walked round-robin
constexpr int kPieceBytes = 32 * 128;
constexpr int kCUs = 256;
constexpr int kNQ = 256;
constexpr int kDim = 128;

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)

// A piece: row i at i * 128, its 16-B quad q rotated within the row so that each ds_read_b128 lane group (lanes {0-3, 12-15,
// 20-27} and {4-11, 16-19, 28-31} of each wave half) covers the 64 banks once.
//   32x32x32 (the screen's ring layout): a group reads 16 different rows at ONE quad -> quad (q - (i >> 1)) & 7;
//   16x16x64: a group reads rows {0-3, 12-15} at quad q and rows 4-11 at quad q +- 1 -> quad (q - (i & 6)) & 7
//   (row pairs 0..7 then sit at q - {0, 2, 4, 6, 0, 2, 4, 6}, and with the +-1 of pairs 2-5 all eight differ; q - (i >> 1) would
//   collide two-way).  Rows 16 apart share a rotation in either layout.
template <bool S16>
__host__ __device__ inline int quad_off(int row, int quad) {
    return row * 128 + (((quad - (S16 ? (row & 6) : (row >> 1))) * 16) & 112);
}

template <bool S16>
__global__ __launch_bounds__(kWaves * 64, 1) void body(const i32x4* __restrict__ asrc, const i32x4* __restrict__ bsrc,
                                                       const int* __restrict__ thr, uint32_t* __restrict__ out,
                                                       uint64_t* __restrict__ stamps, int iters) {
    __shared__ __attribute__((aligned(16))) char smem[kWaves * kNS * kPieceBytes];
    __shared__ int thr_lds[kNQ];      // 16x16x64: 16 thresholds per lane do not fit beside 64 accumulators, read per block
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* const lds = smem + wave * (kNS * kPieceBytes);
    const i32x4* const src = asrc + (size_t)(blockIdx.x * kWaves + wave) * (kNS * kPieceBytes / 16);
    for (int o = lane; o < kNS * kPieceBytes / 16; o += 64) reinterpret_cast<i32x4*>(lds)[o] = src[o];

    constexpr int NC = S16 ? 16 : 8;     // query blocks (of 16 or 32 queries)
    constexpr int KS = S16 ? 2 : 4;      // k-steps (of 64 or 32 bytes)
    constexpr int NCH = NC / 2;          // query blocks per half
    const int col = S16 ? (lane & 15) : (lane & 31);
    const int grp = S16 ? (lane >> 4) : (lane >> 5);
    i32x4 bfrag[NC][KS];
    int thr_s[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bfrag[c][ks] = bsrc[(c * KS + ks) * 64 + lane];
            asm volatile("" : "+a"(bfrag[c][ks]));
        }
        if (!S16) {
            thr_s[c] = thr[c * 32 + col];
            asm volatile("" : "+v"(thr_s[c]));
        }
    }
    if (S16 && threadIdx.x < kNQ) thr_lds[threadIdx.x] = thr[threadIdx.x];
    // 16x16x64: fragment j = 2 * rh + ks is row (lane & 15) + 16 * rh, quad 4 * ks + (lane >> 4); rows 16 apart share a
    // rotation, so the second row half is the first + 2 KiB.  32x32x32: fragment j = ks is row lane & 31, quad 2 * ks + (lane >> 5)
    constexpr int NRD = S16 ? 2 : 4;
    int rd[NRD];
#pragma unroll
    for (int j = 0; j < NRD; ++j) {
        rd[j] = quad_off<S16>(col, S16 ? 4 * j + grp : 2 * j + grp);
        asm volatile("" : "+v"(rd[j]));      // one address register per fragment, not its terms
    }
    __syncthreads();

    uint32_t cnt = 0, chk = 0;
    // hits of one lane in one query block, bit r of mask = register r: count them, and sum (row + 1) * (query + 1) with
    // row = base - 1 + (r & 3) + step * (r >> 2), from bit counts (no per-register factor stays live across the loop)
    auto tally = [&](uint32_t mask, uint32_t q, uint32_t base, uint32_t step) {
        const uint32_t n = __builtin_popcount(mask);
        const uint32_t lo = __builtin_popcount(mask & 0xaaaau) + 2 * __builtin_popcount(mask & 0xccccu);
        const uint32_t hi = __builtin_popcount(mask & 0xf0f0u) + 2 * __builtin_popcount(mask & 0xff00u);
        cnt += n;
        chk += (n * base + lo + step * hi) * (q + 1);
    };
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int b = 0; b < iters; ++b) {
        asm volatile("" ::: "memory");
        const char* slot = lds + (b % kNS) * kPieceBytes;
        i32x4 a4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a4[j] = *reinterpret_cast<const i32x4*>(slot + (S16 ? rd[j & 1] + 2048 * (j >> 1) : rd[j]));
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            __builtin_amdgcn_sched_barrier(0);      // one half's accumulators at a time
            uint64_t cmask[NCH];
            bool hit[NCH];
            uint64_t any_mask = 0;
            if constexpr (S16) {
                i32x4 acc[2][NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) thr_s[half * NCH + c] = thr_lds[(half * NCH + c) * 16 + col];
#pragma unroll
                for (int rh = 0; rh < 2; ++rh)
#pragma unroll
                    for (int c = 0; c < NCH; ++c) acc[rh][c] = i32x4{0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    // all 16 accumulators per k-step, so an accumulator's second MFMA never waits for its first; a query block's
                    // two row halves finish together, so its test can start under the remaining MFMAs
#pragma unroll
                    for (int c = 0; c < NCH; ++c)
#pragma unroll
                        for (int rh = 0; rh < 2; ++rh)
                            acc[rh][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a4[2 * rh + ks], bfrag[half * NCH + c][ks], acc[rh][c], 0, 0, 0);
                    if (ks == 0) __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    int m = acc[0][c][0];
#pragma unroll
                    for (int r = 1; r < 8; ++r) m = acc[r >> 2][c][r & 3] > m ? acc[r >> 2][c][r & 3] : m;
                    hit[c] = m >= thr_s[half * NCH + c];
                    cmask[c] = __builtin_amdgcn_ballot_w64(hit[c]);
                    any_mask |= cmask[c];
                }
                if (any_mask != 0) {
                    uint32_t z = 0;      // opaque: the lane's column and group are rebuilt here, not kept live across the loop
                    asm volatile("" : "+v"(z));
                    const uint32_t l2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
                    const uint32_t colv = l2 & 15, grpv = l2 >> 4;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        if (cmask[c] == 0 || !hit[c]) continue;
                        const uint32_t q = (half * NCH + c) * 16 + colv;
                        uint32_t mask = 0;
#pragma unroll
                        for (int r = 0; r < 8; ++r) mask |= (uint32_t)(acc[r >> 2][c][r & 3] >= thr_s[half * NCH + c]) << r;
                        // D[m][n] of the 16x16 shape: n = lane & 15, m = 4 * (lane >> 4) + register, second row half + 16
                        tally(mask, q, 4 * grpv + 1, 16);
                    }
                }
            } else {
                i32x16 acc[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[c][r] = 0;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int c = 0; c < NCH; ++c)
                        acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a4[ks], bfrag[half * NCH + c][ks], acc[c], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    int m = acc[c][0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) m = acc[c][r] > m ? acc[c][r] : m;
                    hit[c] = m >= thr_s[half * NCH + c];
                    cmask[c] = __builtin_amdgcn_ballot_w64(hit[c]);
                    any_mask |= cmask[c];
                }
                if (any_mask != 0) {
                    uint32_t z = 0;      // opaque: the lane's column and group are rebuilt here, not kept live across the loop
                    asm volatile("" : "+v"(z));
                    const uint32_t l2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
                    const uint32_t colv = l2 & 31, grpv = l2 >> 5;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        if (cmask[c] == 0 || !hit[c]) continue;
                        const uint32_t q = (half * NCH + c) * 32 + colv;
                        uint32_t mask = 0;
#pragma unroll
                        for (int r = 0; r < 16; ++r) mask |= (uint32_t)(acc[c][r] >= thr_s[half * NCH + c]) << r;
                        // D[m][n] of the 32x32 shape: n = lane & 31, m = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
                        tally(mask, q, 4 * grpv + 1, 8);
                    }
                }
            }
        }
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (cnt) {
        atomicAdd(&out[blockIdx.x * 2], cnt);
        atomicAdd(&out[blockIdx.x * 2 + 1], chk);
    }
    if (threadIdx.x == 0) {
        stamps[blockIdx.x * 2] = t1 - t0;
        stamps[blockIdx.x * 2 + 1] = r1 - r0;
    }
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}
static int8_t rand_i8() { return (int8_t)((int)(rng() % 255u) - 127); }

struct Variant {
    const char* name;
    bool s16;
    i32x4* a;
    i32x4* b;
    uint32_t* out;
    std::vector<double> ms, cyc, ghz;
};

static void launch(const Variant& v, const int* thr, uint64_t* stamps, int iters) {
    if (v.s16) body<true><<<kCUs, kWaves * 64>>>(v.a, v.b, thr, v.out, stamps, iters);
    else body<false><<<kCUs, kWaves * 64>>>(v.a, v.b, thr, v.out, stamps, iters);
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 12;
    const int launches = argc > 2 ? atoi(argv[2]) : 30;
    const int iters = (argc > 3 ? atoi(argv[3]) : 3000) / kNS * kNS;
    if (rounds < 1 || launches < 1 || iters < kNS) {
        fprintf(stderr, "usage: %s [rounds] [launches per round] [blocks per wave]\n", argv[0]);
        return 2;
    }

    const size_t a_bytes = (size_t)kCUs * kWaves * kNS * kPieceBytes;
    std::vector<int8_t> ha(a_bytes), ha_img[2], hq(kNQ * kDim);      // ha: pieces of 32 rows x 128, row-major
    for (auto& x : ha) x = rand_i8();
    for (int i = 0; i < 2; ++i) {
        ha_img[i].resize(a_bytes);
        for (size_t p = 0; p < a_bytes / kPieceBytes; ++p)
            for (int m = 0; m < 32; ++m)
                for (int k = 0; k < kDim; ++k)
                    ha_img[i][p * kPieceBytes + (i ? quad_off<true>(m, k >> 4) : quad_off<false>(m, k >> 4)) + (k & 15)] =
                        ha[p * kPieceBytes + m * kDim + k];
    }
    for (auto& x : hq) x = rand_i8();
    // sigma of a K = 128 dot product of uniform [-127, 127] integers: (255^2 - 1) / 12 * sqrt(128) = 61 306
    std::vector<int> hthr(kNQ);
    for (int q = 0; q < kNQ; ++q) hthr[q] = (int)(61306.0 * (3.7 + 0.002 * q));
    // B fragments, [c][ks][lane] x 16 B.  32x32x32: query 32c + (lane & 31), bytes 32ks + 16(lane >> 5) ..+15;
    // 16x16x64: query 16c + (lane & 15), bytes 64ks + 16(lane >> 4) ..+15
    std::vector<int8_t> hb32(kNQ * kDim), hb16(kNQ * kDim);
    for (int c = 0; c < 8; ++c)
        for (int ks = 0; ks < 4; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j)
                    hb32[((c * 4 + ks) * 64 + l) * 16 + j] = hq[(32 * c + (l & 31)) * kDim + 32 * ks + 16 * (l >> 5) + j];
    for (int c = 0; c < 16; ++c)
        for (int ks = 0; ks < 2; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j)
                    hb16[((c * 2 + ks) * 64 + l) * 16 + j] = hq[(16 * c + (l & 15)) * kDim + 64 * ks + 16 * (l >> 4) + j];

    int* thr;
    uint64_t* stamps;
    Variant v[2] = {{"32x32x32", false, nullptr, nullptr, nullptr, {}, {}, {}}, {"16x16x64", true, nullptr, nullptr, nullptr, {}, {}, {}}};
    CHECK(hipMalloc(&thr, kNQ * sizeof(int)));
    CHECK(hipMemcpy(thr, hthr.data(), kNQ * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&stamps, kCUs * 2 * sizeof(uint64_t)));
    for (int i = 0; i < 2; ++i) {
        CHECK(hipMalloc(&v[i].a, a_bytes));
        CHECK(hipMemcpy(v[i].a, ha_img[i].data(), a_bytes, hipMemcpyHostToDevice));
        CHECK(hipMalloc(&v[i].b, kNQ * kDim));
        CHECK(hipMemcpy(v[i].b, (i ? hb16 : hb32).data(), kNQ * kDim, hipMemcpyHostToDevice));
        CHECK(hipMalloc(&v[i].out, kCUs * 2 * sizeof(uint32_t)));
    }

    // ---- layouts: one pass over the ring per variant, against each other and (workgroup 0) against the host
    std::vector<uint32_t> ho[2];
    for (int i = 0; i < 2; ++i) {
        CHECK(hipMemset(v[i].out, 0, kCUs * 2 * sizeof(uint32_t)));
        launch(v[i], thr, stamps, kNS);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        ho[i].resize(kCUs * 2);
        CHECK(hipMemcpy(ho[i].data(), v[i].out, kCUs * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    uint32_t ref_cnt = 0, ref_chk = 0;
    for (int p = 0; p < kWaves * kNS; ++p)
        for (int m = 0; m < 32; ++m)
            for (int q = 0; q < kNQ; ++q) {
                int dot = 0;
                for (int k = 0; k < kDim; ++k)
                    dot += (int)ha[(size_t)p * kPieceBytes + m * kDim + k] * (int)hq[q * kDim + k];
                if (dot >= hthr[q]) {
                    ++ref_cnt;
                    ref_chk += (uint32_t)(m + 1) * (uint32_t)(q + 1);
                }
            }
    uint64_t hits = 0;
    bool same = true;
    for (int i = 0; i < kCUs * 2; ++i) same = same && ho[0][i] == ho[1][i];
    for (int i = 0; i < kCUs; ++i) hits += ho[0][2 * i];
    const bool ok = same && ho[0][0] == ref_cnt && ho[0][1] == ref_chk && ho[1][0] == ref_cnt && ho[1][1] == ref_chk;
    printf("layout check: workgroup 0 hits host %u / 32x32x32 %u / 16x16x64 %u, checksum %08x / %08x / %08x, all %d workgroups %s: %s\n",
           ref_cnt, ho[0][0], ho[1][0], ref_chk, ho[0][1], ho[1][1], kCUs, same ? "equal" : "DIFFER", ok ? "ok" : "FAILED");
    printf("hit (row, query) pairs per 32-row block: %.3f\n", (double)hits / (kCUs * kWaves * kNS));
    if (!ok) return 1;

    // ---- ~2 s of back-to-back launches, then alternating rounds
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float warm_ms = 0.0f;
    while (warm_ms < 2000.0f) {
        CHECK(hipEventRecord(e0));
        for (int l = 0; l < 10; ++l) launch(v[l & 1], thr, stamps, iters);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        warm_ms += ms;
    }
    std::vector<uint64_t> hs(kCUs * 2);
    for (int r = 0; r < rounds; ++r)
        for (int j = 0; j < 2; ++j) {
            Variant& x = v[(r + j) & 1];             // the variant that goes first alternates too
            CHECK(hipEventRecord(e0));
            for (int l = 0; l < launches; ++l) launch(x, thr, stamps, iters);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            CHECK(hipMemcpy(hs.data(), stamps, kCUs * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));      // the round's last launch
            std::vector<double> c(kCUs), g(kCUs);
            for (int i = 0; i < kCUs; ++i) {
                c[i] = (double)hs[2 * i];
                g[i] = hs[2 * i + 1] ? (double)hs[2 * i] / (double)hs[2 * i + 1] * 0.1 : 0.0;      // s_memrealtime ticks at 100 MHz
            }
            x.ms.push_back(ms / launches);
            x.cyc.push_back(median(c) / iters);
            x.ghz.push_back(median(g));
        }

    printf("%d rounds x %d launches x %d blocks per wave, %d workgroups x %d waves, random int8 operands\n", rounds, launches, iters, kCUs, kWaves);
    printf("%-10s %12s %12s %12s %16s %14s %12s\n", "shape", "median ms", "min ms", "max ms", "cycles / block", "in-kernel GHz", "Tops/s (med)");
    for (int i = 0; i < 2; ++i) {
        const double med = median(v[i].ms);
        const double ops = 2.0 * 32 * kNQ * kDim * (double)iters * kCUs * kWaves;
        printf("%-10s %12.4f %12.4f %12.4f %16.1f %14.3f %12.1f\n", v[i].name, med, *std::min_element(v[i].ms.begin(), v[i].ms.end()),
               *std::max_element(v[i].ms.begin(), v[i].ms.end()), median(v[i].cyc), median(v[i].ghz), ops / med / 1e9);
    }
    printf("per round ms (32x32x32 | 16x16x64):");
    for (int r = 0; r < rounds; ++r) printf(" %.4f|%.4f", v[0].ms[r], v[1].ms[r]);
    printf("\n");
    const double med16 = median(v[1].ms), best32 = *std::min_element(v[0].ms.begin(), v[0].ms.end());
    printf("decision: 16x16x64 median %.4f ms vs best 32x32x32 round %.4f ms (ratio %.4f): %s\n", med16, best32, med16 / best32,
           med16 < best32 ? "GO" : "NO-GO");
    return 0;
}
