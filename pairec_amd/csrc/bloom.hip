// bloom.hip — User2ItemExposureBloomFilter on the device: one Bloom bitset per user in HBM, tested over the
// candidate lists of cand_lists.hpp between the fan-in and rank, added to after the page is returned.  What an answer is —
// the hash, the locations, Redis's bit order, the key store's packing, the host statements — is bloom_host.hpp's; this file
// holds the two objects, the kernels and the entry points.
//
// The reference: filter/user_item_exposure_bloom_filter.go:92-98 keeps the items whose Exists is false; filter/bloomfilter/
// bloom.go:67-96 turns a value into k locations; redis_bitset.go:31-44 sets them, :46-108 tests them.
//
// A slot holds the Redis string's bytes as they are, so a 32-bit little-endian load of word N >> 5 has bit N at (N & 31) ^ 7
// (bloom_word_bit).  Slots lie at a stride of bloom_slot_stride(m) bytes, a multiple of 256; slot offsets are 64-bit (40 slots
// of 2^30 bits pass 4 GiB).
//
// Kernels:
//   bloom_probe_kernel<kBytes>   256 lanes per workgroup, grid (cap / 256, nq), one lane per candidate.  The lane loads its row,
//                                its key descriptor and the key's <= 16 words (issued together), mixes each word once — the
//                                block mix of murmur3 does not see the seed — then per seed folds, finalises, reduces by % m and
//                                issues the word load; only then are the k words tested.  Each probe is a random 4-byte read into
//                                a bitset of up to 512 MiB: the stage is bound by random-line latency, so it is spread over the
//                                chip even at nq = 1 and a lane's k loads are in flight at once.  kBytes: Exists as bytes
//                                (pg_bloom_exists_dev); else one keep ballot per wave into kSlotBloom.
//   bloom_compact_kernel         one workgroup of 1 024 lanes per request walks the ballot words in order (block_rank.hpp's
//                                chunk_rank: one barrier per chunk), cand_carry and cand_pad as item_state_filter_kernel.
//   bloom_add_kernel             the probe's grid and location arithmetic, then one agent-scope atomic OR per location.
#include "cand_lists.hpp"
#include "block_rank.hpp"
#include "bloom_host.hpp"

#include <memory>

struct pg_bloom_keys {
    int device = 0;
    uint64_t rows = 0;
    uint64_t* d_desc = nullptr;          // [rows] (word offset << 8) | length
    uint32_t* d_words = nullptr;         // the keys' words, bloom_keys_pack's
};

struct pg_bloom {
    int device = 0;
    uint32_t m = 0, k = 0, n_slots = 0;
    uint32_t seeds[pg::kBloomMaxK] = {0};
    uint64_t stride = 0;                 // bytes between slots
    uint8_t* d_bits = nullptr;           // [n_slots][stride]
};

namespace pg {
namespace {

static_assert(kBloomMaxQueries == (uint32_t)kMaxQueries && kBloomMaxCap == kCandMaxCap && kBloomPadRow == kCandPad,
              "bloom_host.hpp repeats these without cand_lists.hpp");

constexpr uint32_t kBloomThreads = 256;
constexpr uint32_t kBloomChunk = 1024, kBloomWaves = kBloomChunk / kWave;

struct BloomDev {
    const uint8_t* bits;
    uint64_t stride;
    uint32_t m, k, n_slots;
    uint32_t seeds[kBloomMaxK];
    const uint64_t* desc;
    const uint32_t* words;
    uint64_t key_rows;
};

// the words' mixes and the length of the key of `row` (a lane with no key: length 0, every mix 0).  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t bloom_load_key(const BloomDev& b, bool has_key, unsigned long long row, uint32_t* mixed) {
    uint32_t len = 0;
    uint64_t off = 0;
    if (has_key) {
        const uint64_t d = b.desc[row];
        len = (uint32_t)(d & 0xFFu);
        off = d >> 8;
    }
    // Every load is unconditional at a safe address (a lane past its key reads words[0], which always exists) and the branch
    // around it is wave-uniform — the longest key of the wave decides — so no load waits for the one before it.
    const uint32_t nw = (len + 3u) >> 2;
    uint32_t w[kBloomKeyWords];
#pragma unroll
    for (uint32_t i = 0; i < kBloomKeyWords; ++i) {
        w[i] = 0u;
        if (__ballot(i < nw) != 0ull) w[i] = b.words[i < nw ? off + i : 0ull];
    }
#pragma unroll
    for (uint32_t i = 0; i < kBloomKeyWords; ++i) mixed[i] = i < nw ? bloom_mix(w[i]) : 0u;
    return len;
}
// murmur3's body over the mixes with constant register indices; a block past the key's folds nothing
__device__ __forceinline__ uint32_t bloom_hash_reg(const uint32_t* mixed, uint32_t len, uint32_t seed) {
    uint32_t h = seed;
    const uint32_t nblocks = len >> 2;
    uint32_t tail = 0;
#pragma unroll
    for (uint32_t i = 0; i < kBloomKeyWords; ++i) {
        if (i < nblocks) h = bloom_fold(h, mixed[i]);
        if (i == nblocks) tail = mixed[i];
    }
    if (len & 3u) h ^= tail;
    return bloom_fmix(h, len);
}

// what every kernel asks of position pos of request q: a real entry?  one to probe (a key and a slot)?
struct BloomEntry {
    bool real, probe;
    unsigned long long row;
    uint32_t slot;
};
__device__ __forceinline__ BloomEntry bloom_entry(const BloomDev& b, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ count,
                                                  const uint32_t* __restrict__ slots, uint32_t cap, uint32_t q, uint32_t pos) {
    BloomEntry e{false, false, kCandPad, kBloomNoSlot};
    if (pos >= cap) return e;
    const uint32_t n_valid = count ? min(count[q], cap) : cap;
    e.row = rows[(size_t)q * cap + pos];
    e.slot = slots[q];
    e.real = pos < n_valid && e.row != kCandPad;
    e.probe = e.real && e.row < b.key_rows && e.slot < b.n_slots;    // (kBloomNoSlot is >= every n_slots)
    return e;
}

// Request q = blockIdx.y, positions blockIdx.x * 256 ...
template <bool kBytes>
__global__ __launch_bounds__(kBloomThreads) void bloom_probe_kernel(BloomDev b, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ count,
                                                                     const uint32_t* __restrict__ slots, uint32_t cap,
                                                                     unsigned long long* __restrict__ out_ballot, uint8_t* __restrict__ out_exists) {
    const uint32_t q = blockIdx.y, pos = blockIdx.x * kBloomThreads + threadIdx.x;
    const BloomEntry e = bloom_entry(b, rows, count, slots, cap, q, pos);
    uint32_t mixed[kBloomKeyWords];
    const uint32_t len = bloom_load_key(b, e.probe, e.row, mixed);
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(b.bits + (e.probe ? (uint64_t)e.slot * b.stride : 0ull));
    // The k word loads leave together: the only branch around them is on k, which is uniform, and a lane with nothing to probe
    // loads word 0 of slot 0 (always there) and ignores it.  A seed past k loads nothing and tests as "set".
    uint32_t word[kBloomMaxK], bit[kBloomMaxK];
#pragma unroll
    for (uint32_t j = 0; j < kBloomMaxK; ++j) {
        word[j] = ~0u;
        bit[j] = 1u;
        if (j < b.k) {
            const uint32_t loc = bloom_hash_reg(mixed, len, b.seeds[j]) % b.m;      // (< m: inside slot 0 as inside any slot)
            bit[j] = bloom_word_bit(loc);
            word[j] = bits[e.probe ? loc >> 5 : 0u];
        }
    }
    bool all = true;
#pragma unroll
    for (uint32_t j = 0; j < kBloomMaxK; ++j) all = all && (word[j] & bit[j]) != 0u;
    const bool exists = e.probe && all;
    if constexpr (kBytes) {
        if (pos < cap) out_exists[(size_t)q * cap + pos] = exists ? 1 : 0;
    } else {
        const unsigned long long keep = __ballot(e.real && !exists);
        const uint32_t n_words = (cap + kWave - 1) / kWave, wi = pos / kWave;
        if ((threadIdx.x & (kWave - 1)) == 0 && wi < n_words) out_ballot[(size_t)q * n_words + wi] = keep;
    }
}

__global__ __launch_bounds__(kBloomThreads) void bloom_add_kernel(BloomDev b, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ count,
                                                                   const uint32_t* __restrict__ slots, uint32_t cap) {
    const uint32_t q = blockIdx.y, pos = blockIdx.x * kBloomThreads + threadIdx.x;
    const BloomEntry e = bloom_entry(b, rows, count, slots, cap, q, pos);
    uint32_t mixed[kBloomKeyWords];
    const uint32_t len = bloom_load_key(b, e.probe, e.row, mixed);
    if (!e.probe) return;
    uint32_t* bits = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(b.bits) + (uint64_t)e.slot * b.stride);
#pragma unroll
    for (uint32_t j = 0; j < kBloomMaxK; ++j) {
        if (j < b.k) {
            const uint32_t loc = bloom_hash_reg(mixed, len, b.seeds[j]) % b.m;
            __hip_atomic_fetch_or(bits + (loc >> 5), bloom_word_bit(loc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Request q = blockIdx.x: the probe's ballots → the kept entries at the front, everything carried, padding behind the count
__global__ __launch_bounds__(kBloomChunk) void bloom_compact_kernel(CandIn in, CandOut out, const unsigned long long* __restrict__ ballot) {
    __shared__ uint32_t wcnt[2 * kBloomWaves];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const size_t q0 = (size_t)q * in.cap;
    const uint32_t n_valid = cand_n_valid(in, q);
    const uint32_t n_words = (in.cap + kWave - 1) / kWave;
    uint32_t run = 0;
    for (uint32_t c0 = 0, it = 0; c0 < n_valid; c0 += kBloomChunk, ++it) {
        const uint32_t pos = c0 + tid, wi = c0 / kWave + wave;
        const unsigned long long m = wi < n_words ? ballot[(size_t)q * n_words + wi] : 0ull;
        const bool keep = (m >> lane) & 1ull;                              // (the probe kept nothing at or behind n_valid)
        uint32_t r, total;
        chunk_rank<kBloomWaves>(keep, wcnt, it, &r, &total);
        if (keep) cand_carry(in, out, q0 + pos, q0 + run + r, true);       // (run + r <= pos < cap)
        run += total;
    }
    cand_pad(in, out, q, run + tid, kBloomChunk, kCandNan);
    if (tid == 0) out.count[q] = run;
}

BloomDev bloom_dev(const pg_bloom* b, const pg_bloom_keys* keys) {
    BloomDev d{};
    d.bits = b->d_bits;
    d.stride = b->stride;
    d.m = b->m;
    d.k = b->k;
    d.n_slots = b->n_slots;
    memcpy(d.seeds, b->seeds, sizeof d.seeds);
    d.desc = keys->d_desc;
    d.words = keys->d_words;
    d.key_rows = keys->rows;
    return d;
}

int bloom_refuse(const BloomRefusal& r) {
    set_error("%s", r.msg);
    return r.code;
}

int bloom_check_objects(const pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, const char* who) {
    PG_REQUIRE(b->device == ctx->device && keys->device == ctx->device, "%s: the filter (device %d) and the keys (device %d) must live on the context's device %d",
               who, b->device, keys->device, ctx->device);
    return PG_OK;
}

inline dim3 bloom_grid(uint32_t nq, uint32_t cap) { return dim3((cap + kBloomThreads - 1) / kBloomThreads, nq); }
inline size_t bloom_ballot_words(uint32_t nq, uint32_t cap) { return (size_t)nq * ((cap + kWave - 1) / kWave); }

// caller holds ctx->mu; enqueue only
int bloom_exists_locked(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const uint32_t* d_count, const uint32_t* d_slots, uint8_t* d_out) {
    bloom_probe_kernel<true><<<bloom_grid(nq, cap), kBloomThreads, 0, ctx->stream>>>(bloom_dev(b, keys), d_rows, d_count, d_slots, cap, nullptr, d_out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
int bloom_add_locked(pg_ctx* ctx, pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows, const uint32_t* d_count,
                     const uint32_t* d_slots) {
    bloom_add_kernel<<<bloom_grid(nq, cap), kBloomThreads, 0, ctx->stream>>>(bloom_dev(b, keys), d_rows, d_count, d_slots, cap);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
// ballot: bloom_ballot_words(nq, cap) words of device memory (NULL: kSlotBloom is carved here)
int bloom_filter_locked(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, const CandIn& in, const CandOut& out, const uint32_t* d_slots,
                        unsigned long long* ballot) {
    int rc;
    if (!ballot && (rc = scratch_carve(ctx, kSlotBloom, [&](Carve& c) { ballot = c.take<unsigned long long>(bloom_ballot_words(in.nq, in.cap)); })))
        return rc;
    bloom_probe_kernel<false><<<bloom_grid(in.nq, in.cap), kBloomThreads, 0, ctx->stream>>>(bloom_dev(b, keys), in.rows, in.count, d_slots, in.cap, ballot,
                                                                                           nullptr);
    PG_HIP(hipGetLastError());
    bloom_compact_kernel<<<in.nq, kBloomChunk, 0, ctx->stream>>>(in, out, ballot);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int bloom_keys_upload(pg_ctx* ctx, uint64_t rows, const uint64_t* offsets, const uint8_t* bytes, const char* who, pg_bloom_keys** out) {
    BloomKeysPacked pk;
    bloom_keys_pack(rows, offsets, bytes, &pk);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<pg_bloom_keys> ks(new pg_bloom_keys());
    ks->device = ctx->device;
    ks->rows = rows;
    const size_t desc_bytes = std::max<size_t>(rows, 1) * 8, word_bytes = pk.words.size() * 4;
    if (hipMalloc((void**)&ks->d_desc, desc_bytes) != hipSuccess || hipMalloc((void**)&ks->d_words, word_bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (ks->d_desc) (void)hipFree(ks->d_desc);
        set_error("%s: hipMalloc(%.1f MB) failed", who, (double)(desc_bytes + word_bytes) / 1e6);
        return PG_ERR_NOMEM;
    }
    hipError_t e = rows ? hipMemcpyAsync(ks->d_desc, pk.desc.data(), rows * 8, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(ks->d_words, pk.words.data(), word_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(ks->d_desc);
        (void)hipFree(ks->d_words);
        set_error("%s: the upload failed: %s", who, hipGetErrorString(e));
        return PG_ERR_DEVICE;
    }
    *out = ks.release();
    return PG_OK;
}

// the checks the host statements share, in the device entries' order where they have a counterpart
int bloom_host_bind(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, const uint8_t* bitsets, uint64_t key_rows, const uint64_t* key_offsets,
                    const uint8_t* key_bytes, const char* who, BloomHost* b, BloomKeysHost* ks) {
    BloomRefusal r;
    if (!bloom_check_params(m, k, who, &r)) return bloom_refuse(r);
    PG_REQUIRE(n_slots == 0 || bitsets, "%s: NULL argument", who);
    if (!bloom_keys_validate(key_rows, key_offsets, key_bytes, who, &r)) return bloom_refuse(r);
    b->m = (uint32_t)m;
    b->k = k;
    b->n_slots = n_slots;
    bloom_seeds(seeds, k, b->seeds);
    b->bits = const_cast<uint8_t*>(bitsets);
    ks->rows = key_rows;
    ks->offsets = key_offsets;
    ks->bytes = key_bytes;
    return PG_OK;
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_bloom_estimate(uint64_t n, double p, uint64_t* m, uint32_t* k) {
    PG_REQUIRE(m && k, "pg_bloom_estimate: NULL argument");
    PG_REQUIRE(pg::bloom_estimate(n, p, m, k), "pg_bloom_estimate: n=%llu, p=%g (n >= 1, 0 < p < 1)", (unsigned long long)n, p);
    return PG_OK;
}

int pg_bloom_murmur3_host(const uint8_t* bytes, uint64_t n, uint32_t seed, uint32_t* out) {
    PG_REQUIRE(out && (n == 0 || bytes), "pg_bloom_murmur3_host: NULL argument");
    *out = pg::bloom_murmur3(bytes, n, seed);
    return PG_OK;
}

int pg_bloom_keys_create(pg_ctx* ctx, uint64_t rows, const uint64_t* offsets, const uint8_t* bytes, pg_bloom_keys** out) {
    const char* who = "pg_bloom_keys_create";
    PG_REQUIRE(ctx && offsets && out, "%s: NULL argument", who);
    pg::BloomRefusal r;
    if (!pg::bloom_keys_validate(rows, offsets, bytes, who, &r)) return pg::bloom_refuse(r);
    return pg::bloom_keys_upload(ctx, rows, offsets, bytes, who, out);
}

int pg_bloom_keys_create_decimal(pg_ctx* ctx, uint64_t rows, const int64_t* ids, pg_bloom_keys** out) {
    const char* who = "pg_bloom_keys_create_decimal";
    PG_REQUIRE(ctx && out && (rows == 0 || ids), "%s: NULL argument", who);
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> bytes;
    pg::bloom_keys_decimal(rows, ids, &offsets, &bytes);
    return pg::bloom_keys_upload(ctx, rows, offsets.data(), bytes.data(), who, out);
}

int pg_bloom_keys_free(pg_ctx* ctx, pg_bloom_keys* keys) {
    PG_REQUIRE(ctx, "pg_bloom_keys_free: ctx is NULL");
    if (!keys) return PG_OK;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(keys->d_desc);
        (void)hipFree(keys->d_words);
    }
    delete keys;
    return PG_OK;
}

int pg_bloom_create(pg_ctx* ctx, uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, pg_bloom** out) {
    const char* who = "pg_bloom_create";
    PG_REQUIRE(ctx && out, "%s: NULL argument", who);
    pg::BloomRefusal r;
    if (!pg::bloom_check_params(m, k, who, &r)) return pg::bloom_refuse(r);
    PG_REQUIRE(n_slots >= 1, "%s: n_slots=0", who);
    std::unique_ptr<pg_bloom> b(new pg_bloom());
    b->device = ctx->device;
    b->m = (uint32_t)m;
    b->k = k;
    b->n_slots = n_slots;
    pg::bloom_seeds(seeds, k, b->seeds);
    b->stride = pg::bloom_slot_stride(b->m);
    const uint64_t total = b->stride * n_slots;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    if (hipMalloc((void**)&b->d_bits, total) != hipSuccess) {
        (void)hipGetLastError();
        pg::set_error("%s: hipMalloc(%.1f MB) failed", who, (double)total / 1e6);
        return PG_ERR_NOMEM;
    }
    if (hipMemsetAsync(b->d_bits, 0, total, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(b->d_bits);
        pg::set_error("%s: clearing the slots failed", who);
        return PG_ERR_DEVICE;
    }
    *out = b.release();
    return PG_OK;
}

int pg_bloom_free(pg_ctx* ctx, pg_bloom* b) {
    PG_REQUIRE(ctx, "pg_bloom_free: ctx is NULL");
    if (!b) return PG_OK;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        PG_HIP(hipSetDevice(ctx->device));
        PG_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(b->d_bits);
    }
    delete b;
    return PG_OK;
}

int pg_bloom_info(const pg_bloom* b, uint64_t* m, uint32_t* k, uint32_t* n_slots, uint64_t* slot_bytes) {
    PG_REQUIRE(b, "pg_bloom_info: NULL argument");
    if (m) *m = b->m;
    if (k) *k = b->k;
    if (n_slots) *n_slots = b->n_slots;
    if (slot_bytes) *slot_bytes = b->stride;
    return PG_OK;
}

int pg_bloom_slot_write(pg_ctx* ctx, pg_bloom* b, uint32_t slot, const uint8_t* bytes, uint64_t n) {
    const char* who = "pg_bloom_slot_write";
    PG_REQUIRE(ctx && b && (n == 0 || bytes), "%s: NULL argument", who);
    pg::BloomRefusal r;
    if (!pg::bloom_check_slot(slot, b->n_slots, n, b->m, who, &r)) return pg::bloom_refuse(r);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    uint8_t* d = b->d_bits + (uint64_t)slot * b->stride;
    const uint64_t nb = pg::bloom_bytes(b->m);
    // the caller's bytes as they are but for the last byte of the bitset, whose bits at or above m are cleared; zero behind them
    uint8_t last = 0;
    const bool has_last = n == nb;
    if (has_last) last = bytes[nb - 1] & pg::bloom_last_byte_mask(b->m);
    const uint64_t plain = has_last ? nb - 1 : n;
    if (plain) PG_HIP(hipMemcpyAsync(d, bytes, plain, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipMemsetAsync(d + plain, 0, b->stride - plain, ctx->stream));
    if (has_last) PG_HIP(hipMemcpyAsync(d + nb - 1, &last, 1, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_bloom_slot_read(pg_ctx* ctx, const pg_bloom* b, uint32_t slot, uint8_t* bytes, uint64_t n) {
    const char* who = "pg_bloom_slot_read";
    PG_REQUIRE(ctx && b && (n == 0 || bytes), "%s: NULL argument", who);
    pg::BloomRefusal r;
    if (!pg::bloom_check_slot(slot, b->n_slots, n, b->m, who, &r)) return pg::bloom_refuse(r);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    if (n) PG_HIP(hipMemcpyAsync(bytes, b->d_bits + (uint64_t)slot * b->stride, n, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_bloom_slot_clear(pg_ctx* ctx, pg_bloom* b, uint32_t slot) {
    const char* who = "pg_bloom_slot_clear";
    PG_REQUIRE(ctx && b, "%s: NULL argument", who);
    pg::BloomRefusal r;
    if (!pg::bloom_check_slot(slot, b->n_slots, 0, b->m, who, &r)) return pg::bloom_refuse(r);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    PG_HIP(hipMemsetAsync(b->d_bits + (uint64_t)slot * b->stride, 0, b->stride, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_bloom_exists_dev(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const uint32_t* d_count, const uint32_t* d_slots, uint8_t* d_out_exists) {
    const char* who = "pg_bloom_exists_dev";
    PG_REQUIRE(ctx && b && keys && d_rows && d_slots && d_out_exists, "%s: NULL argument", who);
    int rc;
    if ((rc = pg::bloom_check_objects(ctx, b, keys, who)) || (rc = pg::cand_check_nq(nq, who))) return rc;
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::bloom_exists_locked(ctx, b, keys, nq, cap, d_rows, d_count, d_slots, d_out_exists);
}

int pg_bloom_add_dev(pg_ctx* ctx, pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                     const uint32_t* d_count, const uint32_t* d_slots) {
    const char* who = "pg_bloom_add_dev";
    PG_REQUIRE(ctx && b && keys && d_rows && d_slots, "%s: NULL argument", who);
    int rc;
    if ((rc = pg::bloom_check_objects(ctx, b, keys, who)) || (rc = pg::cand_check_nq(nq, who))) return rc;
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::bloom_add_locked(ctx, b, keys, nq, cap, d_rows, d_count, d_slots);
}

// pg_item_state_filter_dev's checks in its order (cond.hip): the required pointers, the stage's own object, the shape, the stage's
// own per-request input, the optional arrays, the overlaps
int pg_bloom_filter_dev(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64, uint32_t n_f64,
                        const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, const uint32_t* d_slots,
                        uint64_t* d_out_rows, double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64,
                        uint32_t* d_out_source_mask, float* d_out_planes_f32, uint32_t* d_out_count) {
    const char* who = "pg_bloom_filter_dev";
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    int rc;
    if ((rc = pg::cand_call_required(l, ctx && b && keys, who))) return rc;
    if ((rc = pg::bloom_check_objects(ctx, b, keys, who))) return rc;
    if ((rc = pg::cand_check_nq(nq, who))) return rc;
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    PG_REQUIRE(d_slots, "%s: d_slots is needed (PG_BLOOM_NO_SLOT for a user without history)", who);
    if ((rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) || (rc = pg::cand_call_apart(l, nq, cap, cap, who))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::bloom_filter_locked(ctx, b, keys, in, out, d_slots, nullptr);
}

// ---- one request on host arrays (staged_run, cand_lists.hpp) ---------------------------------------------------------------------
int pg_bloom_exists(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t n, const uint64_t* rows, uint32_t slot,
                    uint8_t* out_exists) {
    const char* who = "pg_bloom_exists";
    PG_REQUIRE(ctx && b && keys && (n == 0 || (rows && out_exists)), "%s: NULL argument", who);
    int rc;
    if ((rc = pg::bloom_check_objects(ctx, b, keys, who))) return rc;
    if (n == 0) return PG_OK;                        // an empty request: an empty answer
    if (n > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, n, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kBallot, kRows, kSlot, kOut };
    Staged st[] = {{nullptr, 0, Staged::kSkip, pg::bloom_ballot_words(1, n) * 8}, {rows, (size_t)n * 8, Staged::kIn}, {&slot, 4, Staged::kIn},
                   {out_exists, n, Staged::kOut}};
    return pg::staged_run(ctx, pg::kSlotBloom, st, sizeof st / sizeof *st, true /* slot is this frame's */, [&] {
        return pg::bloom_exists_locked(ctx, b, keys, 1, n, st[kRows].at<uint64_t>(), nullptr, st[kSlot].at<uint32_t>(), st[kOut].at<uint8_t>());
    });
}

int pg_bloom_add(pg_ctx* ctx, pg_bloom* b, const pg_bloom_keys* keys, uint32_t n, const uint64_t* rows, uint32_t slot) {
    const char* who = "pg_bloom_add";
    PG_REQUIRE(ctx && b && keys && (n == 0 || rows), "%s: NULL argument", who);
    int rc;
    if ((rc = pg::bloom_check_objects(ctx, b, keys, who))) return rc;
    if (n == 0) return PG_OK;                        // an empty page: nothing to add
    if (n > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, n, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kBallot, kRows, kSlot };
    Staged st[] = {{nullptr, 0, Staged::kSkip, pg::bloom_ballot_words(1, n) * 8}, {rows, (size_t)n * 8, Staged::kIn}, {&slot, 4, Staged::kIn}};
    return pg::staged_run(ctx, pg::kSlotBloom, st, sizeof st / sizeof *st, true /* slot is this frame's */, [&] {
        return pg::bloom_add_locked(ctx, b, keys, 1, n, st[kRows].at<uint64_t>(), nullptr, st[kSlot].at<uint32_t>());
    });
}

int pg_bloom_filter(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t n, const uint64_t* rows, const double* score,
                    const uint8_t* source, uint32_t slot, uint64_t* out_rows, double* out_score, uint8_t* out_source, uint32_t* out_count) {
    const char* who = "pg_bloom_filter";
    PG_REQUIRE(ctx && b && keys && out_count && (n == 0 || (rows && score && out_rows && out_score)), "%s: NULL argument", who);
    PG_REQUIRE(!source == !out_source, "%s: source and out_source come in pairs", who);
    int rc;
    if ((rc = pg::bloom_check_objects(ctx, b, keys, who))) return rc;
    if (n == 0) {                                    // an empty request: an empty answer
        *out_count = 0;
        return PG_OK;
    }
    if (n > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, n, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kBallot, kRows, kScore, kOutRows, kOutScore, kSource, kOutSource, kSlot, kCount };
    Staged st[] = {{nullptr, 0, Staged::kSkip, pg::bloom_ballot_words(1, n) * 8},
                   {rows, (size_t)n * 8, Staged::kIn},       {score, (size_t)n * 8, Staged::kIn},   {out_rows, (size_t)n * 8, Staged::kOut},
                   {out_score, (size_t)n * 8, Staged::kOut}, {source, n, Staged::in_if(source)},    {out_source, n, Staged::out_if(source)},
                   {&slot, 4, Staged::kIn},                  {out_count, 4, Staged::kOut}};
    return pg::staged_run(ctx, pg::kSlotBloom, st, sizeof st / sizeof *st, true /* slot is this frame's */, [&] {
        pg::CandIn in{};
        in.rows = st[kRows].at<uint64_t>();
        in.score = st[kScore].at<unsigned long long>();
        in.source = source ? st[kSource].at<uint8_t>() : nullptr;
        in.nq = 1;
        in.cap = n;
        pg::CandOut out{};
        out.rows = st[kOutRows].at<uint64_t>();
        out.score = st[kOutScore].at<unsigned long long>();
        out.source = source ? st[kOutSource].at<uint8_t>() : nullptr;
        out.count = st[kCount].at<uint32_t>();
        out.out_cap = n;
        return pg::bloom_filter_locked(ctx, b, keys, in, out, st[kSlot].at<uint32_t>(), st[kBallot].at<unsigned long long>());
    });
}

// ---- the host statements (bloom_host.hpp) behind the same checks --------------------------------------------------------------------
int pg_bloom_exists_host(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, const uint8_t* bitsets, uint64_t key_rows,
                         const uint64_t* key_offsets, const uint8_t* key_bytes, uint32_t nq, uint32_t cap, const uint64_t* rows,
                         const uint32_t* count, const uint32_t* slots, uint8_t* out_exists) {
    const char* who = "pg_bloom_exists_host";
    PG_REQUIRE(key_offsets && rows && slots && out_exists, "%s: NULL argument", who);
    pg::BloomHost b;
    pg::BloomKeysHost ks;
    int rc;
    if ((rc = pg::bloom_host_bind(m, k, seeds, n_slots, bitsets, key_rows, key_offsets, key_bytes, who, &b, &ks))) return rc;
    if ((rc = pg::cand_check_nq(nq, who))) return rc;
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    pg::bloom_exists_host(b, ks, nq, cap, rows, count, slots, out_exists);
    return PG_OK;
}

int pg_bloom_add_host(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, uint8_t* bitsets, uint64_t key_rows,
                      const uint64_t* key_offsets, const uint8_t* key_bytes, uint32_t nq, uint32_t cap, const uint64_t* rows,
                      const uint32_t* count, const uint32_t* slots) {
    const char* who = "pg_bloom_add_host";
    PG_REQUIRE(key_offsets && rows && slots, "%s: NULL argument", who);
    pg::BloomHost b;
    pg::BloomKeysHost ks;
    int rc;
    if ((rc = pg::bloom_host_bind(m, k, seeds, n_slots, bitsets, key_rows, key_offsets, key_bytes, who, &b, &ks))) return rc;
    if ((rc = pg::cand_check_nq(nq, who))) return rc;
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    pg::bloom_add_host(b, ks, nq, cap, rows, count, slots);
    return PG_OK;
}

int pg_bloom_filter_host(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, const uint8_t* bitsets, uint64_t key_rows,
                         const uint64_t* key_offsets, const uint8_t* key_bytes, uint32_t nq, uint32_t cap, const uint64_t* rows,
                         const double* score, const uint8_t* source, const uint32_t* count, const double* planes_f64, uint32_t n_f64,
                         const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32, const uint32_t* slots, uint64_t* out_rows,
                         double* out_score, uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32,
                         uint32_t* out_count) {
    const char* who = "pg_bloom_filter_host";
    const pg::CandCall l{rows, score, source, count, planes_f64, n_f64, source_mask, planes_f32, n_f32, out_rows, out_score,
                         out_source, out_planes_f64, out_source_mask, out_planes_f32, out_count};
    int rc;
    if ((rc = pg::cand_call_required(l, key_offsets != nullptr, who))) return rc;
    pg::BloomHost b;
    pg::BloomKeysHost ks;
    if ((rc = pg::bloom_host_bind(m, k, seeds, n_slots, bitsets, key_rows, key_offsets, key_bytes, who, &b, &ks))) return rc;
    if ((rc = pg::cand_check_nq(nq, who))) return rc;
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("%s: cap=%u unsupported (1..%u)", who, cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    PG_REQUIRE(slots, "%s: slots is needed (PG_BLOOM_NO_SLOT for a user without history)", who);
    if ((rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) || (rc = pg::cand_call_apart(l, nq, cap, cap, who))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, cap, &in, &out);
    std::vector<uint8_t> keep((size_t)nq * cap);
    pg::bloom_keep_host(b, ks, nq, cap, rows, count, slots, keep.data());
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t q0 = (size_t)q * cap;
        uint32_t run = 0;
        for (uint32_t p = 0; p < cap; ++p)
            if (keep[q0 + p]) pg::cand_carry(in, out, q0 + p, q0 + run++, true);
        pg::cand_pad(in, out, q, run, 1, pg::kCandNan);
        out_count[q] = run;
    }
    return PG_OK;
}

int pg_bloom_slot_write_host(uint64_t m, uint32_t n_slots, uint8_t* bitsets, uint32_t slot, const uint8_t* bytes, uint64_t n) {
    const char* who = "pg_bloom_slot_write_host";
    PG_REQUIRE(bitsets && (n == 0 || bytes), "%s: NULL argument", who);
    pg::BloomRefusal r;
    if (!pg::bloom_check_params(m, 1, who, &r) || !pg::bloom_check_slot(slot, n_slots, n, (uint32_t)m, who, &r)) return pg::bloom_refuse(r);
    pg::bloom_slot_write_host((uint32_t)m, bitsets + (size_t)slot * pg::bloom_bytes((uint32_t)m), bytes, n);
    return PG_OK;
}

}  // extern "C"
