// ColdStartRecall on the device: the rows a WhereClause admits turned into a recall answer, in the two orders
// the reference serves (module/cold_start_recall_hologres_dao.go:76-80) — a uniform random sample per request (`ORDER BY
// random() LIMIT n`) and the head of the pool by a column (`ORDER BY create_time DESC LIMIT n`).  coldstart_host.hpp states the
// answer (parser, keys, permutation, host statement); this file holds what computes it over up to 2^32 - 1 rows:
//
//   prefix   admitted rows per 1 024-row block of the clause's bitmap and their exclusive scan, built once per bitmap epoch and
//            kept by the pg_cold beside the reference that keeps the bitmap alive;
//   sample   one lane per output slot: P(i) -> binary search in the prefix -> the block's words by popcount -> the bit;
//   select   the exact k-th key of the admitted rows by eight most-significant-digit passes (LDS histogram per workgroup, one
//            global add per non-empty bin, a one-workgroup pick that keeps the threshold on the device), then ONE ordered
//            collection — every row better than the threshold key and the first t rows of the threshold key in row order, placed
//            by per-block counts and a scan — and the order of the <= k survivors by split_sort.hpp's runs and merge (up to
//            8 192 of them; counting ranks above).
#include "common.hpp"
#include "block_rank.hpp"
#include "coldstart_host.hpp"
#include "split_sort.hpp"

namespace pg {
namespace {

constexpr uint32_t kColdBlockRows = 1024, kColdBlockWords = kColdBlockRows / 32;     // where.hip's kWhereBlockRows
constexpr uint32_t kScanChunk = 1024;                                                // elements a workgroup scans

// the kept (bitmap, prefix) pair of one binding; a call holds a reference while it enqueues, a replacement waits for the device
struct ColdState {
    std::shared_ptr<void> hold;          // the clause's bitmap (where.hip's), nullptr when the bitmap is our own (no clause)
    const uint32_t* bits = nullptr;
    uint32_t* prefix = nullptr;          // [blocks] admitted rows before block b
    void* d = nullptr;                   // prefix, the scan's chunk sums and, without a clause, the all-ones bitmap
    int device = -1;
    uint64_t rows = 0, admitted = 0, epoch = 0;
    size_t bytes = 0;
    ~ColdState() { if (d) (void)hipFree(d); }
};

struct ColdSel {                         // the select's state: the threshold key's digits chosen so far, the places still to fill
    unsigned long long prefix;
    uint32_t remaining, pad;
};

}  // namespace
}  // namespace pg

struct pg_cold {
    const pg_where* w = nullptr;         // borrowed
    pg::ColdSpec spec;
    mutable std::mutex mu;               // serialises the prefix builds; guards cur and st
    mutable std::shared_ptr<pg::ColdState> cur;
    mutable pg_cold_stats_t st{};
};

namespace pg {
namespace {

constexpr uint32_t kColdWaves = 256 / kWave;                                         // every kernel here: 256 lanes; a scan's ws: 4 elements of LDS

// ---- exclusive scan of n elements in place: chunk sums, their scan by one workgroup, the chunks -----------------------------
template <class T>
__global__ __launch_bounds__(256) void scan_sums_kernel(const T* __restrict__ in, uint32_t n, T* __restrict__ sums) {
    __shared__ T ws[4];
    const uint32_t i0 = blockIdx.x * kScanChunk + threadIdx.x * 4;
    T s = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) s += i0 + j < n ? in[i0 + j] : (T)0;
    T total;
    (void)block_excl_scan<kColdWaves>(s, ws, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
template <class T>
__global__ __launch_bounds__(256) void scan_top_kernel(T* __restrict__ sums, uint32_t m) {
    __shared__ T ws[4];
    T carry = 0;
    for (uint32_t base = 0; base < m; base += 256) {          // (uniform trip count)
        const uint32_t i = base + threadIdx.x;
        const T v = i < m ? sums[i] : (T)0;
        T total;
        const T ex = block_excl_scan<kColdWaves>(v, ws, &total);
        if (i < m) sums[i] = carry + ex;
        carry += total;
        __syncthreads();                                      // (the next round's scan writes ws again)
    }
}
template <class T>
__global__ __launch_bounds__(256) void scan_apply_kernel(T* __restrict__ io, uint32_t n, const T* __restrict__ sums) {
    __shared__ T ws[4];
    const uint32_t i0 = blockIdx.x * kScanChunk + threadIdx.x * 4;
    T v[4], s = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        v[j] = i0 + j < n ? io[i0 + j] : (T)0;
        s += v[j];
    }
    T total;
    T ex = block_excl_scan<kColdWaves>(s, ws, &total) + sums[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (i0 + j < n) io[i0 + j] = ex;
        ex += v[j];
    }
}
inline uint32_t scan_chunks(uint32_t n) { return (n + kScanChunk - 1) / kScanChunk; }
// sums: scan_chunks(n) elements of scratch
template <class T>
int scan_launch(hipStream_t s, T* io, uint32_t n, T* sums) {
    const uint32_t m = scan_chunks(n);
    scan_sums_kernel<T><<<m, 256, 0, s>>>(io, n, sums);
    scan_top_kernel<T><<<1, 256, 0, s>>>(sums, m);
    scan_apply_kernel<T><<<m, 256, 0, s>>>(io, n, sums);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// ---- prefix ------------------------------------------------------------------------------------------------------------------
// the bitmap of a pool without a clause: every row of the table
__global__ __launch_bounds__(256) void cold_ones_kernel(uint32_t* __restrict__ bits, uint64_t rows, uint32_t words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    const uint64_t left = rows - (uint64_t)i * 32;
    bits[i] = left >= 32 ? ~0u : (1u << (uint32_t)left) - 1u;
}
// 32 lanes per block of 1 024 rows: a word each, coalesced
__global__ __launch_bounds__(256) void cold_block_count_kernel(const uint32_t* __restrict__ bits, uint32_t words, uint32_t blocks,
                                                               uint32_t* __restrict__ counts) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t blk = g >> 5, w = g;                       // (word blk * 32 + (g & 31) == g)
    uint32_t c = blk < blocks && w < words ? (uint32_t)__popc(bits[w]) : 0u;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((g & 31u) == 0 && blk < blocks) counts[blk] = c;
}

// ---- sample --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cold_sample_kernel(const uint32_t* __restrict__ bits, uint32_t words, const uint32_t* __restrict__ prefix,
                                                          uint32_t blocks, uint64_t A, uint32_t h, const unsigned long long* __restrict__ seed,
                                                          uint32_t nq, uint32_t k, uint32_t kk, uint64_t row_offset,
                                                          unsigned long long* __restrict__ out_rows, float* __restrict__ out_scores,
                                                          uint32_t* __restrict__ out_count) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nq * k) return;
    const uint32_t q = g / k, i = g - q * k;
    if (i == 0 && out_count) out_count[q] = kk;
    if (i >= kk) {
        out_rows[g] = ~0ull;
        out_scores[g] = -__builtin_inff();
        return;
    }
    const uint32_t j = (uint32_t)cold_perm(seed ? seed[q] : 0ull, A, h, i);
    uint32_t lo = 0, hi = blocks;                             // the last block whose prefix is <= j
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= j) lo = mid; else hi = mid;
    }
    uint32_t rem = j - prefix[lo], w = lo * kColdBlockWords, word = 0;
    const uint32_t w_end = min(w + kColdBlockWords, words);
    for (; w < w_end; ++w) {
        word = bits[w];
        const uint32_t c = (uint32_t)__popc(word);
        if (rem < c) break;
        rem -= c;
    }
    for (; rem; --rem) word &= word - 1u;                     // the rem-th set bit
    const uint32_t bit = word ? (uint32_t)__ffs(word) - 1u : 0u;
    out_rows[g] = row_offset + (uint64_t)min(w, w_end - 1) * 32 + bit;
    out_scores[g] = 0.0f;
}

// ---- select --------------------------------------------------------------------------------------------------------------------
// The four rows r0 .. r0 + 3 (r0 a multiple of 4) of a lane: which are admitted (the return's bits 0-3) and their keys, the
// column read only where a row is — 16-B loads for a whole group.
__device__ inline uint32_t cold_load4(const uint32_t* __restrict__ bits, const void* __restrict__ col, int dtype, bool desc, uint64_t rows,
                                      uint64_t r0, unsigned long long key[4]) {
    if (r0 >= rows) return 0u;
    const uint32_t valid = r0 + 4 <= rows ? 0xFu : (1u << (uint32_t)(rows - r0)) - 1u;
    const uint32_t nib = (bits[r0 >> 5] >> (uint32_t)(r0 & 31u)) & valid;
    if (!nib) return 0u;
    unsigned long long raw[4] = {0, 0, 0, 0};
    if (dtype == PG_F_I64 || dtype == PG_F_F64) {
        const unsigned long long* c = reinterpret_cast<const unsigned long long*>(col) + r0;
        if (valid == 0xFu) {
            const ulonglong2 a = reinterpret_cast<const ulonglong2*>(c)[0], b = reinterpret_cast<const ulonglong2*>(c)[1];
            raw[0] = a.x; raw[1] = a.y; raw[2] = b.x; raw[3] = b.y;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 3; ++j) if ((valid >> j) & 1u) raw[j] = c[j];
        }
    } else {
        const uint32_t* c = reinterpret_cast<const uint32_t*>(col) + r0;
        if (valid == 0xFu) {
            const uint4 a = *reinterpret_cast<const uint4*>(c);
            raw[0] = a.x; raw[1] = a.y; raw[2] = a.z; raw[3] = a.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 3; ++j) if ((valid >> j) & 1u) raw[j] = c[j];
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) key[j] = cold_key_raw(dtype, raw[j], desc);
    return nib;
}

__global__ __launch_bounds__(256) void cold_sel_init_kernel(ColdSel* __restrict__ st, uint32_t* __restrict__ hist, uint32_t kk) {
    hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st->prefix = 0;
        st->remaining = kk;
        st->pad = 0;
    }
}

// Digit `shift / 8` of the admitted rows whose higher digits are the threshold's so far.  A wave whose rows all carry one digit —
// every wave of a high pass over real data, every wave of a column of equal values — adds its count once instead of 64 times
// to one LDS address; the block then adds each non-empty bin to the global histogram once.
__global__ __launch_bounds__(256) void cold_hist_kernel(const uint32_t* __restrict__ bits, const void* __restrict__ col, int dtype, int desc,
                                                        uint64_t rows, const ColdSel* __restrict__ st, uint32_t shift,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    lh[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix;
    const uint64_t tiles = (rows + kColdBlockRows - 1) / kColdBlockRows;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {          // (uniform over the block: every lane reaches the ballots)
        unsigned long long key[4] = {0, 0, 0, 0};
        const uint32_t nib = cold_load4(bits, col, dtype, desc != 0, rows, tile * kColdBlockRows + tid * 4, key);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const bool on = ((nib >> j) & 1u) && (shift == 56 || ((key[j] ^ prefix) >> (shift + 8)) == 0);
            const uint32_t digit = (uint32_t)(key[j] >> shift) & 255u;
            const unsigned long long am = __ballot(on);
            if (!am) continue;
            const int leader = __ffsll(am) - 1;
            const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
            const unsigned long long same = __ballot(on && digit == d0);
            if (same == am) {
                if ((int)lane == leader) atomicAdd(&lh[d0], (uint32_t)__popcll(am));
            } else if (on) {
                atomicAdd(&lh[digit], 1u);
            }
        }
    }
    __syncthreads();
    if (lh[tid]) atomicAdd(&hist[tid], lh[tid]);
}

// one workgroup: the bin that holds the `remaining`-th key in ascending order becomes the threshold's next digit
__global__ __launch_bounds__(256) void cold_pick_kernel(uint32_t* __restrict__ hist, ColdSel* __restrict__ st, uint32_t shift) {
    __shared__ uint32_t ws[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t c = hist[tid];
    hist[tid] = 0;                                            // (the next pass's)
    const uint32_t rem = st->remaining;
    uint32_t total;
    const uint32_t ex = block_excl_scan<kColdWaves>(c, ws, &total);  // (its barrier stands between every lane's read of the state and the write)
    if (c && ex < rem && rem <= ex + c) {
        st->prefix |= (unsigned long long)tid << shift;
        st->remaining = rem - ex;
    }
}

// per tile of 1 024 rows: the rows better than the threshold key (high half) and the rows of the threshold key (low half)
__global__ __launch_bounds__(256) void cold_tile_count_kernel(const uint32_t* __restrict__ bits, const void* __restrict__ col, int dtype, int desc,
                                                              uint64_t rows, const ColdSel* __restrict__ st,
                                                              unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long ws[4];
    const unsigned long long T = st->prefix;
    unsigned long long key[4] = {0, 0, 0, 0};
    const uint32_t nib = cold_load4(bits, col, dtype, desc != 0, rows, (uint64_t)blockIdx.x * kColdBlockRows + threadIdx.x * 4, key);
    unsigned long long v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if ((nib >> j) & 1u) v += key[j] < T ? (1ull << 32) : key[j] == T ? 1ull : 0ull;
    unsigned long long total;
    (void)block_excl_scan<kColdWaves>(v, ws, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
// scan: the tile counts' exclusive scan.  The better rows fill [0, kk - t) in row order, the first t rows of the threshold key
// [kk - t, kk) in row order: no atomics, the tie rule is part of the answer.
__global__ __launch_bounds__(256) void cold_collect_kernel(const uint32_t* __restrict__ bits, const void* __restrict__ col, int dtype, int desc,
                                                           uint64_t rows, const ColdSel* __restrict__ st,
                                                           const unsigned long long* __restrict__ scan, uint32_t kk,
                                                           unsigned long long* __restrict__ skey, uint32_t* __restrict__ srow) {
    __shared__ unsigned long long ws[4];
    const unsigned long long T = st->prefix;
    const uint32_t t_take = st->remaining;
    const uint64_t r0 = (uint64_t)blockIdx.x * kColdBlockRows + threadIdx.x * 4;
    unsigned long long key[4] = {0, 0, 0, 0};
    const uint32_t nib = cold_load4(bits, col, dtype, desc != 0, rows, r0, key);
    unsigned long long v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if ((nib >> j) & 1u) v += key[j] < T ? (1ull << 32) : key[j] == T ? 1ull : 0ull;
    unsigned long long total;
    const unsigned long long at = scan[blockIdx.x] + block_excl_scan<kColdWaves>(v, ws, &total);
    uint32_t bpos = (uint32_t)(at >> 32), tpos = (uint32_t)at;
    const uint32_t n_better = kk - min(t_take, kk);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (!((nib >> j) & 1u)) continue;
        uint32_t pos = ~0u;
        if (key[j] < T) pos = bpos++;
        else if (key[j] == T) { if (tpos < t_take) pos = n_better + tpos; ++tpos; }
        if (pos < kk) {
            skey[pos] = key[j];
            srow[pos] = (uint32_t)(r0 + j);
        }
    }
}
// The survivors' order.  Each group was collected in row order and every better row's key is below the threshold's, so (key,
// then row) is (key, then position): the order split_sort.hpp's runs and merge produce, for up to kSplitMaxItems survivors.
struct ColdSortPolicy {
    static constexpr bool kWithIdx = true;
    const unsigned long long* skey;
    const uint32_t* srow;
    uint32_t n;
    uint32_t* ordered;
    __device__ uint32_t count(uint32_t) const { return n; }
    __device__ uint64_t key(uint32_t, uint32_t i) const { return skey[i]; }
    __device__ void store(uint32_t, uint32_t rank, uint64_t, uint32_t ix) const { ordered[rank] = srow[ix]; }
    __device__ void tail(uint32_t, uint32_t, uint32_t, uint32_t) const {}
};
// ... and above that (the split sort's runs no longer fit LDS) by counting, as the recalls' final order does there: rank =
// survivors that come before (key, then row); rows are distinct, ranks a permutation
__global__ __launch_bounds__(256) void cold_rank_kernel(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ srow, uint32_t n,
                                                        uint32_t* __restrict__ ordered) {
    __shared__ unsigned long long lk[256];
    __shared__ uint32_t lr[256];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mk = i < n ? skey[i] : 0ull;
    const uint32_t mr = i < n ? srow[i] : 0u;
    uint32_t rank = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        __syncthreads();
        const uint32_t j = base + threadIdx.x;
        lk[threadIdx.x] = j < n ? skey[j] : ~0ull;
        lr[threadIdx.x] = j < n ? srow[j] : ~0u;
        __syncthreads();
        const uint32_t m = min(256u, n - base);
        for (uint32_t t = 0; t < m; ++t) rank += (lk[t] < mk || (lk[t] == mk && lr[t] < mr)) ? 1u : 0u;
    }
    if (i < n && rank < n) ordered[rank] = mr;
}
// the one list to every request
__global__ __launch_bounds__(256) void cold_fill_kernel(const uint32_t* __restrict__ ordered, uint32_t nq, uint32_t k, uint32_t kk, uint64_t row_offset,
                                                        unsigned long long* __restrict__ out_rows, float* __restrict__ out_scores,
                                                        uint32_t* __restrict__ out_count) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nq * k) return;
    const uint32_t q = g / k, i = g - q * k;
    if (i == 0 && out_count) out_count[q] = kk;
    out_rows[g] = i < kk ? row_offset + ordered[i] : ~0ull;
    out_scores[g] = i < kk ? 0.0f : -__builtin_inff();
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
int cold_state_build(pg_ctx* ctx, uint64_t rows, const WhereServe* ws, std::shared_ptr<ColdState>* out) {
    auto cs = std::make_shared<ColdState>();
    const uint32_t words = (uint32_t)((rows + 31) / 32), blocks = (uint32_t)((rows + kColdBlockRows - 1) / kColdBlockRows);
    const size_t o_sums = align_up((size_t)blocks * 4), o_bits = align_up(o_sums + (size_t)scan_chunks(blocks) * 4);
    const size_t total = o_bits + (ws ? 0 : (size_t)words * 4 + 256);
    PG_HIP(hipSetDevice(ctx->device));
    if (hipMalloc(&cs->d, total) != hipSuccess) {
        (void)hipGetLastError();
        cs->d = nullptr;
        set_error("pg_cold: hipMalloc(%zu) for the prefix of %llu rows failed", total, (unsigned long long)rows);
        return PG_ERR_NOMEM;
    }
    char* d = (char*)cs->d;
    cs->prefix = (uint32_t*)d;
    cs->device = ctx->device;
    cs->rows = rows;
    cs->bytes = total;
    hipStream_t s = ctx->stream;
    if (ws) {
        cs->hold = ws->hold;
        cs->bits = (const uint32_t*)ws->f.col;
        cs->admitted = (uint64_t)ws->f.admitted;
        cs->epoch = ws->id.epoch;
    } else {
        cs->bits = (const uint32_t*)(d + o_bits);
        cs->admitted = rows;
        cold_ones_kernel<<<(words + 255) / 256, 256, 0, s>>>((uint32_t*)(d + o_bits), rows, words);
    }
    cold_block_count_kernel<<<(blocks * kColdBlockWords + 255) / 256, 256, 0, s>>>(cs->bits, words, blocks, cs->prefix);
    int rc = scan_launch<uint32_t>(s, cs->prefix, blocks, (uint32_t*)(d + o_sums));
    // a sibling context that shares the pg_cold reads the prefix from its own stream
    if (rc == PG_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_error("pg_cold: the prefix build failed: %s", hipGetErrorString(hipGetLastError()));
        rc = PG_ERR_DEVICE;
    }
    if (rc != PG_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    *out = std::move(cs);
    return PG_OK;
}

// the current (bitmap, prefix) pair of `c` for `rows` rows of `fs` on ctx's device (caller holds ctx->mu)
int cold_bind(const char* who, pg_ctx* ctx, const pg_cold* c, const pg_features* fs, uint64_t rows, std::shared_ptr<ColdState>* out) {
    int rc;
    std::lock_guard<std::mutex> g(c->mu);
    WhereServe ws;
    if (c->w && (rc = where_bits_bind(who, ctx, c->w, fs, rows, &ws))) return rc;
    std::shared_ptr<ColdState> cs = c->cur;
    const bool hit = cs && cs->device == ctx->device && cs->rows == rows &&
                     (c->w ? cs->epoch == ws.id.epoch && cs->bits == (const uint32_t*)ws.f.col : cs->hold == nullptr);
    if (hit) {
        c->st.prefix_hits++;
    } else {
        if ((rc = cold_state_build(ctx, rows, c->w ? &ws : nullptr, &cs))) return rc;
        // kernels enqueued earlier, on this or a sibling context, may still read the pair this one replaces
        if (c->cur) PG_HIP(hipDeviceSynchronize());
        c->cur = cs;
        c->st.prefix_builds++;
        c->st.bytes = cs->bytes;
        c->st.epoch = cs->epoch;
        c->st.admitted = cs->admitted;
    }
    *out = cs;
    return PG_OK;
}

int cold_order_column(const char* who, const pg_cold* c, const pg_features* fs, const pg_features::Column** out) {
    const pg_features::Column* col = nullptr;
    for (const auto& x : fs->cols)
        if (x.name == c->spec.column) col = &x;
    PG_REQUIRE(col, "%s: the feature store has no column \"%s\"", who, c->spec.column.c_str());
    PG_REQUIRE(col->dtype >= PG_F_I32 && col->dtype <= PG_F_F64 && col->d, "%s: order column \"%s\" must be a numeric column with values", who,
               col->name.c_str());
    *out = col;
    return PG_OK;
}

int cold_check_shape(const char* who, uint32_t nq, uint32_t k) {
    PG_REQUIRE(nq >= 1 && nq <= kColdMaxQueries, "%s: nq=%u must be in [1,%u]", who, nq, kColdMaxQueries);
    if (k < 1 || k > kColdMaxK) {
        set_error("%s: k=%u unsupported (1..%u)", who, k, kColdMaxK);
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}

// every check of pg_cold_recall_dev, on the host, nothing enqueued (no lock needed)
int cold_check(const char* who, const pg_ctx* ctx, const pg_cold* c, const pg_table* t, const pg_features* fs, const void* out_rows,
               const void* out_scores, uint32_t nq, uint32_t k, const pg_features::Column** order_col) {
    PG_REQUIRE(ctx && c && t && out_rows && out_scores, "%s: NULL argument", who);
    const bool ordered = c->spec.order != kColdRandom;
    PG_REQUIRE(fs || !(c->w || ordered), "%s: NULL feature store (the clause and the order column live in one)", who);
    int rc;
    if ((rc = cold_check_shape(who, nq, k))) return rc;
    PG_REQUIRE(!fs || fs->rows >= t->rows, "%s: the feature store holds %llu rows, the table %llu", who, (unsigned long long)(fs ? fs->rows : 0),
               (unsigned long long)t->rows);
    *order_col = nullptr;
    if (ordered && (rc = cold_order_column(who, c, fs, order_col))) return rc;
    if (t->d_row_map || t->rows == 0 || t->rows >= (1ull << 32)) {
        set_error("%s: %s unsupported", who, t->d_row_map ? "a filtered view" : "a table of 0 or >= 2^32 rows");
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}

// the launches (caller holds ctx->mu and the table's shared lock, the checks are made)
int cold_enqueue(const char* who, pg_ctx* ctx, const pg_cold* c, const pg_table* t, const pg_features* fs, const pg_features::Column* order_col,
                 const uint64_t* d_seed, uint32_t nq, uint32_t k, uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count) {
    int rc;
    std::shared_ptr<ColdState> cs;
    if ((rc = cold_bind(who, ctx, c, fs, t->rows, &cs))) return rc;
    PG_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t rows = t->rows, A = cs->admitted;
    const uint32_t words = (uint32_t)((rows + 31) / 32), blocks = (uint32_t)((rows + kColdBlockRows - 1) / kColdBlockRows);
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, A), slots = nq * k;
    if (c->spec.order == kColdRandom) {
        cold_sample_kernel<<<(slots + 255) / 256, 256, 0, s>>>(cs->bits, words, cs->prefix, blocks, A, cold_half_bits(A),
                                                              (const unsigned long long*)d_seed, nq, k, kk, t->row_offset,
                                                              (unsigned long long*)d_out_rows, d_out_scores, d_out_count);
        PG_HIP(hipGetLastError());
        return PG_OK;
    }
    ColdSel* st = nullptr;
    uint32_t *hist = nullptr, *srow = nullptr, *ordered = nullptr;
    unsigned long long *counts = nullptr, *sums = nullptr, *skey = nullptr;
    if ((rc = scratch_carve(ctx, kSlotCold, [&](Carve& cv) {
            st = cv.take<ColdSel>(1);
            hist = cv.take<uint32_t>(256);
            counts = cv.take<unsigned long long>(blocks);
            sums = cv.take<unsigned long long>(scan_chunks(blocks));
            skey = cv.take<unsigned long long>(kk);
            srow = cv.take<uint32_t>(kk);
            ordered = cv.take<uint32_t>(kk);
        }))) return rc;
    if (kk) {
        const int dtype = order_col->dtype, desc = c->spec.order == kColdDesc ? 1 : 0;
        const void* col = order_col->d;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks, (uint64_t)ctx->num_cus * 8);
        cold_sel_init_kernel<<<1, 256, 0, s>>>(st, hist, kk);
        for (uint32_t pass = 0; pass < 8; ++pass) {           // (always eight: a column of equal values costs what any other does)
            const uint32_t shift = 56 - 8 * pass;
            cold_hist_kernel<<<grid, 256, 0, s>>>(cs->bits, col, dtype, desc, rows, st, shift, hist);
            cold_pick_kernel<<<1, 256, 0, s>>>(hist, st, shift);
        }
        cold_tile_count_kernel<<<blocks, 256, 0, s>>>(cs->bits, col, dtype, desc, rows, st, counts);
        if ((rc = scan_launch<unsigned long long>(s, counts, blocks, sums))) return rc;
        cold_collect_kernel<<<blocks, 256, 0, s>>>(cs->bits, col, dtype, desc, rows, st, counts, kk, skey, srow);
        if (kk <= kSplitMaxItems) {
            if ((rc = split_sort_launch(ctx, ColdSortPolicy{skey, srow, kk, ordered}, 1, kk))) return rc;
        } else {
            cold_rank_kernel<<<(kk + 255) / 256, 256, 0, s>>>(skey, srow, kk, ordered);
        }
    }
    cold_fill_kernel<<<(slots + 255) / 256, 256, 0, s>>>(ordered, nq, k, kk, t->row_offset, (unsigned long long*)d_out_rows, d_out_scores,
                                                        d_out_count);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_cold_create(const pg_where* w, const char* order_by, pg_cold** out) {
    PG_REQUIRE(out, "pg_cold_create: NULL argument");
    std::unique_ptr<pg_cold> c(new pg_cold());
    size_t at = 0;
    const char* msg = "";
    if (!pg::cold_parse_order(order_by, &c->spec, &at, &msg)) {
        pg::set_error("pg_cold_create: OrderBy: %s at position %zu", msg, at);
        return PG_ERR_PARSE;
    }
    c->w = w;
    *out = c.release();
    return PG_OK;
}

int pg_cold_free(pg_cold* c) {
    if (c && c->cur) {                                        // (enqueued kernels may still read the pair)
        if (hipSetDevice(c->cur->device) == hipSuccess) (void)hipDeviceSynchronize();
    }
    delete c;
    return PG_OK;
}

int pg_cold_recall_host(const pg_cold* c, const uint32_t* bits, uint64_t rows, uint64_t row_offset, const void* order_col, int order_dtype,
                        const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(c && out_rows && out_scores, "pg_cold_recall_host: NULL argument");
    int rc;
    if ((rc = pg::cold_check_shape("pg_cold_recall_host", nq, k))) return rc;
    if (rows >= (1ull << 32)) {
        pg::set_error("pg_cold_recall_host: %llu rows unsupported", (unsigned long long)rows);
        return PG_ERR_UNSUPPORTED;
    }
    if (c->spec.order != pg::kColdRandom)
        PG_REQUIRE((order_col || rows == 0) && order_dtype >= PG_F_I32 && order_dtype <= PG_F_F64,
                   "pg_cold_recall_host: order column \"%s\" must be a numeric column with values", c->spec.column.c_str());
    pg::cold_recall_host(c->spec.order, bits, rows, row_offset, order_col, order_dtype, seed, nq, k, out_rows, out_scores, out_count);
    return PG_OK;
}

int pg_cold_recall_dev(pg_ctx* ctx, const pg_cold* c, const pg_table* t, const pg_features* fs, const uint64_t* d_seed, uint32_t nq, uint32_t k,
                       uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count) {
    const pg_features::Column* oc;
    int rc;
    if ((rc = pg::cold_check("pg_cold_recall_dev", ctx, c, t, fs, d_out_rows, d_out_scores, nq, k, &oc))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    return pg::cold_enqueue("pg_cold_recall_dev", ctx, c, t, fs, oc, d_seed, nq, k, d_out_rows, d_out_scores, d_out_count);
}

int pg_cold_recall(pg_ctx* ctx, const pg_cold* c, const pg_table* t, const pg_features* fs, const uint64_t* seed, uint32_t nq, uint32_t k,
                   uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    const pg_features::Column* oc;
    int rc;
    if ((rc = pg::cold_check("pg_cold_recall", ctx, c, t, fs, out_rows, out_scores, nq, k, &oc))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    uint64_t *d_seed = nullptr, *d_rows = nullptr;
    float* d_sc = nullptr;
    uint32_t* d_cnt = nullptr;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& cv) {
            d_seed = cv.take<uint64_t>(nq);
            d_rows = cv.take<uint64_t>((size_t)nq * k);
            d_sc = cv.take<float>((size_t)nq * k);
            d_cnt = cv.take<uint32_t>(nq);
        }))) return rc;
    if (seed) PG_HIP(hipMemcpyAsync(d_seed, seed, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = pg::cold_enqueue("pg_cold_recall", ctx, c, t, fs, oc, seed ? d_seed : nullptr, nq, k, d_rows, d_sc, d_cnt);
    if (rc != PG_OK) {
        (void)hipStreamSynchronize(ctx->stream);              // (the seeds' copy reads the caller's memory)
        return rc;
    }
    PG_HIP(hipMemcpyAsync(out_rows, d_rows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(out_scores, d_sc, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_count) PG_HIP(hipMemcpyAsync(out_count, d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_cold_stats(const pg_cold* c, pg_cold_stats_t* out) {
    PG_REQUIRE(c && out, "pg_cold_stats: NULL argument");
    std::lock_guard<std::mutex> g(c->mu);
    *out = c->st;
    return PG_OK;
}

}  // extern "C"
