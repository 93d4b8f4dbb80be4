// block_rank.hpp — the ranks a workgroup's lanes need to move kept entries to the front in order, and the block-wide exclusive
// scan (beside cand_lists.hpp).  Device code only, no state: the callers own the LDS words and say how many
// waves they launch.
//
//   wave_rank      a lane's flag among its wave's flags: the set flags in the lanes before it, and the wave's count
//                  (ballot_rank: the same from a ballot the caller already holds);
//   chunk_rank     the same among the flags of the whole workgroup (one chunk of an ordered walk), with one barrier;
//   block_excl_scan  the exclusive prefix sum of one value per lane over the workgroup, and the sum, with one barrier.
#pragma once
#include "common.hpp"

namespace pg {

// the set bits of a ballot mask in the lanes before this one
__device__ __forceinline__ uint32_t ballot_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// ... of the wave's flags, and their number.  Every active lane of the wave calls it.
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t* count) {
    const unsigned long long m = __ballot(flag);
    *count = (uint32_t)__popcll(m);
    return ballot_rank(m);
}

// The rank of a lane's flag among the flags of a workgroup of WAVES waves, and their number: chunk `it` of a walk.
// wcnt: 2 * WAVES words of LDS that the walk owns, two sets of wave counts; chunk `it` uses set it & 1.
//
// Why two sets and one barrier are enough.  A wave writes its count into set it & 1, passes the barrier, and reads all WAVES
// counts of that set.  A wave that runs ahead into chunk it + 1 writes the OTHER set, so it cannot disturb a wave still reading.
// To write set it & 1 again it must be in chunk it + 2, behind the barrier of chunk it + 1 — and that barrier opens only when
// every wave has reached it, with its reads of chunk it done.  One set would need a second barrier behind the reads.
//
// What a caller may not do: every lane of the workgroup makes every call (the barrier), so a walk ends on conditions that are
// uniform over the workgroup only; between two calls on one wcnt `it` advances by exactly one — only its low bit is read, so
// several walks may share a counter (chunk_rank(.., it++, ..)) — or a barrier of the caller's stands between them; and nothing
// else writes wcnt.
template <uint32_t WAVES>
__device__ __forceinline__ void chunk_rank(bool flag, uint32_t* wcnt, uint32_t it, uint32_t* rank, uint32_t* total) {
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    uint32_t count;
    const uint32_t before = wave_rank(flag, &count);
    uint32_t* wc = wcnt + (it & 1u) * WAVES;
    if (lane == 0) wc[wave] = count;
    __syncthreads();
    uint32_t below = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) {
        const uint32_t c = wc[w];
        below += w < wave ? c : 0u;
        all += c;
    }
    *rank = below + before;
    *total = all;
}

// The exclusive prefix sum of v over a workgroup of WAVES waves in lane order, and the sum of all.  ws: WAVES elements of LDS.
// One barrier, between the waves' sums and their reads; the barrier that lets ws be written again — a second scan, a loop — is
// the caller's.
template <uint32_t WAVES, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* ws, T* total) {
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    T incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T up = __shfl_up(incl, off, kWave);
        if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == kWave - 1) ws[wave] = incl;
    __syncthreads();
    T excl = incl - v, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) {
        const T s = ws[w];
        if (w < wave) excl += s;
        all += s;
    }
    *total = all;
    return excl;
}

}  // namespace pg
