// exclude.hip — per-request exclusion lists applied to a recall's ordered answer.
//
// berecall.User2ItemExposureFilter.BuildQueryParams (service/recall/berecall/user_item_exposure_filter.go:22-33) puts a user's
// exposure_list into the vector query, so that the engine answers with returnCount UNSEEN items; deployments without BE filter
// behind the recall (filter/user_item_exposure_filter.go:34-49, FilterByHistory) and hand rank fewer than RecallCount candidates.
// Here the list never reaches the scan: a recall's answer is totally ordered (score, then row), so the first k entries that are
// not in a list of n ids lie within the first k + n entries of that order.  One ordinary pass at depth k + max n (recall.hip)
// holds every request's exact answer; this file's kernel cuts it out, order preserved, without a sort.
#include "common.hpp"
#include "block_rank.hpp"

namespace pg {
namespace {

constexpr uint32_t kExclSetSlots = 8192;         // open-addressed set of one request's list: at most 4096 ids, load factor <= 0.5
static_assert(kExclSetSlots >= 2 * kMaxExclude, "the set must keep empty slots");
constexpr uint32_t kExclThreads = 1024;          // one workgroup per request; the walk's chunk
constexpr uint32_t kExclWaves = kExclThreads / kWave;
constexpr size_t kExclLds = (size_t)kExclSetSlots * 8 + 2 * kExclWaves * 4;
constexpr unsigned long long kExclEmpty = ~0ull; // never a member: padding is dropped before the set is asked, and never inserted

// (a multiplicative hash: ids that share their low bits — one shard's rows, multiples of the set's size — spread over the set)
__device__ inline uint32_t excl_slot(unsigned long long id) { return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 51); }

// Request q = blockIdx.x: out[q][j] = the j-th entry of in[q][0 .. k_in) that is neither padding (row UINT64_MAX) nor in the
// request's list, j < k_out; the slots behind the kept entries are padding.  Chunks of kExclThreads entries in order: a
// membership test per lane, the lane's place from block_rank.hpp's chunk_rank, and a running base.
// The walk ends with the chunk that fills k_out, so an empty list reads the head only (and builds no set).
__global__ __launch_bounds__(kExclThreads) void exclude_compact_kernel(const uint64_t* __restrict__ rows, const float* __restrict__ scores,
                                                                      uint32_t k_in, const uint64_t* __restrict__ excl,
                                                                      const uint32_t* __restrict__ excl_off, uint32_t k_out, float pad_score,
                                                                      uint64_t* __restrict__ out_rows, float* __restrict__ out_scores,
                                                                      uint32_t* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long excl_set[];      // [kExclSetSlots], then wave counts [2][kExclWaves]
    uint32_t* wcnt = reinterpret_cast<uint32_t*>(excl_set + kExclSetSlots);
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t e0 = excl_off[q];
    // (a longer list breaks the caller's precondition: its first kMaxExclude ids count — the set keeps empty slots, every probe ends)
    const uint32_t n = min(excl_off[q + 1] - e0, kMaxExclude);
    rows += (size_t)q * k_in;
    out_rows += (size_t)q * k_out;
    const uint32_t* sc_bits = reinterpret_cast<const uint32_t*>(scores) + (size_t)q * k_in;
    uint32_t* out_bits = reinterpret_cast<uint32_t*>(out_scores) + (size_t)q * k_out;
    if (n) {
        for (uint32_t i = tid; i < kExclSetSlots; i += kExclThreads) excl_set[i] = kExclEmpty;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kExclThreads) {
            const unsigned long long id = excl[e0 + i];
            if (id == kExclEmpty) continue;
            // (a plain read walks the occupied run, the atomic only claims a slot seen empty: a duplicate finds itself)
            for (uint32_t h = excl_slot(id);; h = (h + 1) & (kExclSetSlots - 1)) {
                unsigned long long cur = excl_set[h];
                if (cur == kExclEmpty) cur = atomicCAS(&excl_set[h], kExclEmpty, id);
                if (cur == kExclEmpty || cur == id) break;
            }
        }
        __syncthreads();
    }
    uint32_t base = 0;
    for (uint32_t c0 = 0, it = 0; c0 < k_in && base < k_out; c0 += kExclThreads, ++it) {
        const uint32_t i = c0 + tid;
        unsigned long long id = kExclEmpty;
        uint32_t bits = 0;
        if (i < k_in) {
            id = rows[i];
            bits = sc_bits[i];
        }
        bool keep = id != kExclEmpty;
        if (keep && n) {
            for (uint32_t h = excl_slot(id);; h = (h + 1) & (kExclSetSlots - 1)) {
                const unsigned long long cur = excl_set[h];
                if (cur == id) keep = false;
                if (cur == id || cur == kExclEmpty) break;
            }
        }
        uint32_t r, total;
        chunk_rank<kExclWaves>(keep, wcnt, it, &r, &total);
        const uint32_t dst = base + r;
        if (keep && dst < k_out) {
            out_rows[dst] = id;
            out_bits[dst] = bits;
        }
        base += total;
    }
    const uint32_t kept = base < k_out ? base : k_out;
    for (uint32_t j = kept + tid; j < k_out; j += kExclThreads) {
        out_rows[j] = kExclEmpty;
        out_scores[(size_t)q * k_out + j] = pad_score;
    }
    if (out_count && tid == 0) out_count[q] = kept;
}

}  // namespace

int exclude_compact_locked(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t k_in,
                           const uint64_t* d_excl_rows, const uint32_t* d_excl_offsets, uint32_t k_out, float pad_score,
                           uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count) {
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)exclude_compact_kernel, kExclLds))) return rc;
    exclude_compact_kernel<<<nq, kExclThreads, kExclLds, ctx->stream>>>(d_rows, d_scores, k_in, d_excl_rows, d_excl_offsets, k_out, pad_score,
                                                                      d_out_rows, d_out_scores, d_out_count);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_exclude_compact_dev(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t k_in,
                           const uint64_t* d_excl_rows, const uint32_t* d_excl_offsets, uint32_t k_out, float pad_score,
                           uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count) {
    PG_REQUIRE(ctx && d_rows && d_scores && d_excl_offsets && d_out_rows && d_out_scores, "pg_exclude_compact_dev: NULL argument");
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)pg::kMaxQueries, "pg_exclude_compact_dev: nq=%u must be in [1,%d]", nq, pg::kMaxQueries);
    if (k_out < 1 || k_out > k_in || k_in > 16384) {
        pg::set_error("pg_exclude_compact_dev: k_out=%u, k_in=%u unsupported (1 <= k_out <= k_in <= 16384)", k_out, k_in);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::exclude_compact_locked(ctx, d_rows, d_scores, nq, k_in, d_excl_rows, d_excl_offsets, k_out, pad_score, d_out_rows,
                                      d_out_scores, d_out_count);
}

}  // extern "C"
