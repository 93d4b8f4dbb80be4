// cf_sort.hpp — the sort of 16-byte records that cf_kernel.hpp (cf.hip, x2i.hip: DESIGN.md 4.1l, 4.1y) and hot.hip (4.1aa) run:
// one workgroup of kCfThreads lanes orders a power-of-two count of (x, y) records ascending, a bitonic network through LDS in
// chunks of kCfSortChunk records with the wider steps in place.  Device code only, no state.
#pragma once
#include "common.hpp"

namespace pg {
namespace {

constexpr uint32_t kCfThreads = 1024;            // one workgroup per request; a list of at most kCfMaxList entries is one entry per lane
constexpr uint32_t kCfSortChunk = 8192;          // 16-byte sort records ordered in LDS at a time (128 KiB, the table's bytes reused)

__device__ inline bool cf_less(const ulonglong2& a, const ulonglong2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

// g[base .. base + n) through LDS: the bitonic network's steps of the merges k_lo .. k_hi whose partner distance is below n
// (n a power of two <= kCfSortChunk; directions follow the global index).
__device__ void cf_sort_lds(ulonglong2* g, ulonglong2* s, uint32_t base, uint32_t n, uint32_t k_lo, uint32_t k_hi) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < n; i += kCfThreads) s[i] = g[base + i];
    __syncthreads();
    for (uint32_t k = k_lo; k <= k_hi && k; k <<= 1) {
        for (uint32_t j = min(k >> 1, n >> 1); j > 0; j >>= 1) {
            for (uint32_t p = tid; p < (n >> 1); p += kCfThreads) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool up = ((base + i) & k) == 0;
                const ulonglong2 x = s[i], y = s[l];
                if (cf_less(y, x) == up) {
                    s[i] = y;
                    s[l] = x;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < n; i += kCfThreads) g[base + i] = s[i];
    __syncthreads();
}

// ascending sort of g[0 .. n), n a power of two: chunks of kCfSortChunk in LDS, the wider steps in place
__device__ void cf_sort(ulonglong2* g, ulonglong2* s, uint32_t n) {
    const uint32_t tid = threadIdx.x;
    if (n <= kCfSortChunk) {
        cf_sort_lds(g, s, 0, n, 2, n);
        return;
    }
    for (uint32_t base = 0; base < n; base += kCfSortChunk) cf_sort_lds(g, s, base, kCfSortChunk, 2, kCfSortChunk);
    for (uint32_t k = kCfSortChunk << 1; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j >= kCfSortChunk; j >>= 1) {
            for (uint32_t p = tid; p < (n >> 1); p += kCfThreads) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const ulonglong2 x = g[i], y = g[l];
                if (cf_less(y, x) == up) {
                    g[i] = y;
                    g[l] = x;
                }
            }
            __syncthreads();
        }
        for (uint32_t base = 0; base < n; base += kCfSortChunk) cf_sort_lds(g, s, base, kCfSortChunk, k, k);
    }
}

}  // namespace
}  // namespace pg
