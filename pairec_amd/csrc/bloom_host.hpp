// bloom_host.hpp — what a User2ItemExposureBloomFilter answer IS, free of HIP: murmur3_x86_32 with a seed, the
// k locations of a key, Redis's bit addressing, the key store's packing and its upload validation, EstimateParameters, and the
// host statements the device kernels reproduce bit for bit.  bloom.hip includes it for both sides; tests/bloom_check.cpp builds
// it with a host compiler alone.
//
// The reference: filter/bloomfilter/bloom.go:67-96 hashes every value to k locations through the user's HashFunc; the one hash
// it shows is bloom_test.go:13-29 — location j of key bytes d is murmur3_x86_32(d, seed_j) % m (spaolacci/murmur3
// New32WithSeed), the seeds the primes of bloom_test.go:14.  redis_bitset.go:31-44 sets the k bits of every value (SETBIT),
// :46-108 tests them (GETBIT: Exists is true when all k are set); bit N of a Redis string is byte N >> 3, mask 0x80 >> (N & 7).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pairec_gpu.h"

#ifdef __HIPCC__
#define PG_BLOOM_HD __host__ __device__ __forceinline__
#else
#define PG_BLOOM_HD inline
#endif

namespace pg {

constexpr uint32_t kBloomMaxKey = 64, kBloomMaxK = 16, kBloomNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kBloomKeyWords = kBloomMaxKey / 4;
constexpr uint32_t kBloomMaxQueries = 256, kBloomMaxCap = 16384;
static_assert(kBloomMaxKey == PG_BLOOM_MAX_KEY && kBloomMaxK == PG_BLOOM_MAX_K && kBloomNoSlot == PG_BLOOM_NO_SLOT,
              "include/pairec_gpu.h states these for the callers");
constexpr unsigned long long kBloomPadRow = ~0ull;                   // the row of a padding entry (cand_lists.hpp's kCandPad)
// the first 16 seeds of bloom_test.go:14
constexpr uint32_t kBloomPrimes[kBloomMaxK] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53};

// ---- murmur3_x86_32 in the three parts the kernels share --------------------------------------------------------------------------
PG_BLOOM_HD uint32_t bloom_rotl(uint32_t x, uint32_t r) { return (x << r) | (x >> (32u - r)); }
// a 4-byte block (or the zero-padded tail) before it meets the hash state: no seed in it, so one mix serves every seed
PG_BLOOM_HD uint32_t bloom_mix(uint32_t k1) {
    k1 *= 0xCC9E2D51u;
    k1 = bloom_rotl(k1, 15);
    return k1 * 0x1B873593u;
}
PG_BLOOM_HD uint32_t bloom_fold(uint32_t h, uint32_t mixed) {
    h ^= mixed;
    h = bloom_rotl(h, 13);
    return h * 5u + 0xE6546B64u;
}
PG_BLOOM_HD uint32_t bloom_fmix(uint32_t h, uint32_t len) {
    h ^= len;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}
// the hash of a key stored as (len + 3) / 4 little-endian words, the last one zero-padded, from the words' mixes
PG_BLOOM_HD uint32_t bloom_hash_mixed(const uint32_t* mixed, uint32_t len, uint32_t seed) {
    uint32_t h = seed;
    const uint32_t nblocks = len >> 2;
    for (uint32_t i = 0; i < nblocks; ++i) h = bloom_fold(h, mixed[i]);
    if (len & 3u) h ^= mixed[nblocks];
    return bloom_fmix(h, len);
}
// murmur3_x86_32 of len bytes at any alignment
inline uint32_t bloom_murmur3(const uint8_t* d, size_t len, uint32_t seed) {
    uint32_t h = seed;
    const size_t nblocks = len >> 2;
    for (size_t i = 0; i < nblocks; ++i) {
        uint32_t w;
        memcpy(&w, d + 4 * i, 4);                                    // (little-endian hosts only, as the device)
        h = bloom_fold(h, bloom_mix(w));
    }
    uint32_t t = 0;
    for (size_t i = 0; i < (len & 3u); ++i) t |= (uint32_t)d[4 * nblocks + i] << (8 * i);
    if (len & 3u) h ^= bloom_mix(t);
    return bloom_fmix(h, (uint32_t)len);
}
// location j of a key (bloom_test.go:21-25)
inline uint32_t bloom_location(const uint8_t* d, size_t len, uint32_t seed, uint32_t m) { return bloom_murmur3(d, len, seed) % m; }

// ---- Redis bit addressing ------------------------------------------------------------------------------------------------------------
// bit N of a Redis string in its bytes ...
PG_BLOOM_HD uint64_t bloom_byte_of(uint32_t n) { return n >> 3; }
PG_BLOOM_HD uint8_t bloom_mask_of(uint32_t n) { return (uint8_t)(0x80u >> (n & 7u)); }
// ... and in the little-endian 32-bit words the device reads the same bytes as: word N >> 5, bit (N & 31) ^ 7
PG_BLOOM_HD uint32_t bloom_word_bit(uint32_t n) { return 1u << ((n & 31u) ^ 7u); }
// bytes of a bitset of m bits, and what the bits at or above m leave of its last byte
PG_BLOOM_HD uint64_t bloom_bytes(uint32_t m) { return ((uint64_t)m + 7u) >> 3; }
PG_BLOOM_HD uint8_t bloom_last_byte_mask(uint32_t m) { return (m & 7u) ? (uint8_t)(0xFF00u >> (m & 7u)) : (uint8_t)0xFFu; }
// a device slot's stride: the bitset's bytes rounded up to 256
PG_BLOOM_HD uint64_t bloom_slot_stride(uint32_t m) { return (bloom_bytes(m) + 255u) & ~(uint64_t)255u; }

// ---- refusals: a code and a message, for callers with their own error convention --------------------------------------------------------
struct BloomRefusal {
    int code = PG_OK;
    char msg[224] = {0};
};
#define PG_BLOOM_REFUSE(r, c, ...)                            \
    do {                                                      \
        (r)->code = (c);                                      \
        snprintf((r)->msg, sizeof (r)->msg, __VA_ARGS__);     \
        return false;                                         \
    } while (0)

// pg_bloom_create's parameters
inline bool bloom_check_params(uint64_t m, uint32_t k, const char* who, BloomRefusal* r) {
    if (m < 1 || m > 0xFFFFFFFFull) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: m=%llu must be in [1, 2^32 - 1]", who, (unsigned long long)m);
    if (k < 1 || k > kBloomMaxK) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: k=%u must be in [1, %u]", who, k, kBloomMaxK);
    return true;
}
// a slot named on the host, and the bytes written to or read from it
inline bool bloom_check_slot(uint32_t slot, uint32_t n_slots, uint64_t n, uint32_t m, const char* who, BloomRefusal* r) {
    if (slot >= n_slots) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: slot %u of %u", who, slot, n_slots);
    if (n > bloom_bytes(m)) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: %llu bytes for a bitset of %llu", who, (unsigned long long)n, (unsigned long long)bloom_bytes(m));
    return true;
}
// the key store's upload validation: offsets [rows + 1] ascend from any start, no key longer than kBloomMaxKey
inline bool bloom_keys_validate(uint64_t rows, const uint64_t* offsets, const uint8_t* bytes, const char* who, BloomRefusal* r) {
    if (!offsets) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: NULL argument", who);
    for (uint64_t i = 0; i < rows; ++i) {
        if (offsets[i + 1] < offsets[i]) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: offsets descend at row %llu", who, (unsigned long long)i);
        if (offsets[i + 1] - offsets[i] > kBloomMaxKey)
            PG_BLOOM_REFUSE(r, PG_ERR_UNSUPPORTED, "%s: the key of row %llu is %llu bytes (at most %u)", who, (unsigned long long)i,
                            (unsigned long long)(offsets[i + 1] - offsets[i]), kBloomMaxKey);
    }
    if (rows && offsets[rows] > offsets[0] && !bytes) PG_BLOOM_REFUSE(r, PG_ERR_INVALID, "%s: NULL argument", who);
    return true;
}

// ---- the key store as the device holds it ---------------------------------------------------------------------------------------------
// Row r: desc[r] = (word offset << 8) | length in bytes; its (length + 3) / 4 words at words[offset ...], the bytes little-endian
// and the last word zero-padded, so that every murmur block is one aligned dword and the tail is the word as it stands.  A
// zero-length key takes no words.  words always holds at least one element.
struct BloomKeysPacked {
    std::vector<uint64_t> desc;
    std::vector<uint32_t> words;
};
inline void bloom_keys_pack(uint64_t rows, const uint64_t* offsets, const uint8_t* bytes, BloomKeysPacked* out) {
    out->desc.resize(rows);
    uint64_t total = 0;
    for (uint64_t i = 0; i < rows; ++i) total += (offsets[i + 1] - offsets[i] + 3) >> 2;
    out->words.assign(total ? total : 1, 0u);
    uint64_t at = 0;
    for (uint64_t i = 0; i < rows; ++i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        out->desc[i] = (at << 8) | len;
        if (len) memcpy(reinterpret_cast<uint8_t*>(out->words.data() + at), bytes + offsets[i], len);
        at += (len + 3) >> 2;
    }
}
// strconv.Itoa of every id, as offsets + bytes (bloom_test.go:49-51)
inline void bloom_keys_decimal(uint64_t rows, const int64_t* ids, std::vector<uint64_t>* offsets, std::vector<uint8_t>* bytes) {
    offsets->assign(rows + 1, 0);
    bytes->clear();
    for (uint64_t i = 0; i < rows; ++i) {
        char buf[24];
        const int n = snprintf(buf, sizeof buf, "%lld", (long long)ids[i]);
        bytes->insert(bytes->end(), buf, buf + n);
        (*offsets)[i + 1] = bytes->size();
    }
}

// ---- EstimateParameters (bloom.go:40-45) --------------------------------------------------------------------------------------------------
// false: n = 0, p outside (0, 1), or an m that a uint32 does not hold
inline bool bloom_estimate(uint64_t n, double p, uint64_t* m, uint32_t* k) {
    if (n < 1 || !(p > 0.0 && p < 1.0)) return false;
    const double mf = std::ceil((double)n * std::log(p) / std::log(1.0 / std::pow(2.0, 0.693147180559945309417232121458176568)));
    const double kf = 0.693147180559945309417232121458176568 * mf / (double)n + 0.5;
    if (!(mf >= 1.0 && mf < 18446744073709551616.0) || !(kf < 4294967296.0)) return false;
    *m = (uint64_t)mf;
    *k = (uint32_t)kf;
    return true;
}

// ---- the host statements -------------------------------------------------------------------------------------------------------------------
// A filter over host bitsets: n_slots Redis strings of bloom_bytes(m) bytes each, one behind the other.
struct BloomHost {
    uint32_t m, k, n_slots;
    uint32_t seeds[kBloomMaxK];
    uint8_t* bits;                       // [n_slots][bloom_bytes(m)]
};
struct BloomKeysHost {
    uint64_t rows;
    const uint64_t* offsets;             // [rows + 1]
    const uint8_t* bytes;
};
inline void bloom_seeds(const uint32_t* seeds, uint32_t k, uint32_t* out) {
    for (uint32_t j = 0; j < kBloomMaxK; ++j) out[j] = j < k ? (seeds ? seeds[j] : kBloomPrimes[j]) : 0u;
}
// is position p of request q a real entry with a key and a slot?  → its row and slot
inline bool bloom_host_entry(const BloomHost& b, const BloomKeysHost& ks, uint32_t cap, const uint64_t* rows, const uint32_t* count,
                             const uint32_t* slots, uint32_t q, uint32_t p, bool* real, uint64_t* row, uint32_t* slot) {
    const uint32_t n_valid = count ? (count[q] < cap ? count[q] : cap) : cap;
    *row = rows[(size_t)q * cap + p];
    *real = p < n_valid && *row != kBloomPadRow;
    *slot = slots[q];
    return *real && *row < ks.rows && *slot < b.n_slots;            // (kBloomNoSlot is >= every n_slots)
}
inline bool bloom_host_test(const BloomHost& b, const BloomKeysHost& ks, uint64_t row, uint32_t slot) {
    const uint8_t* bits = b.bits + (size_t)slot * bloom_bytes(b.m);
    const uint8_t* d = ks.bytes + ks.offsets[row];
    const size_t len = ks.offsets[row + 1] - ks.offsets[row];
    for (uint32_t j = 0; j < b.k; ++j) {
        const uint32_t loc = bloom_location(d, len, b.seeds[j], b.m);
        if (!(bits[bloom_byte_of(loc)] & bloom_mask_of(loc))) return false;
    }
    return true;
}
// Exists alone: out [nq][cap], 1 where all k bits of the entry's key are set in its request's slot; padding, a row outside the
// key store, no slot: 0
inline void bloom_exists_host(const BloomHost& b, const BloomKeysHost& ks, uint32_t nq, uint32_t cap, const uint64_t* rows, const uint32_t* count,
                              const uint32_t* slots, uint8_t* out) {
    for (uint32_t q = 0; q < nq; ++q)
        for (uint32_t p = 0; p < cap; ++p) {
            bool real;
            uint64_t row;
            uint32_t slot;
            out[(size_t)q * cap + p] = bloom_host_entry(b, ks, cap, rows, count, slots, q, p, &real, &row, &slot) && bloom_host_test(b, ks, row, slot) ? 1 : 0;
        }
}
// Add: the k bits of every real entry with a key, in its request's slot
inline void bloom_add_host(const BloomHost& b, const BloomKeysHost& ks, uint32_t nq, uint32_t cap, const uint64_t* rows, const uint32_t* count,
                           const uint32_t* slots) {
    for (uint32_t q = 0; q < nq; ++q)
        for (uint32_t p = 0; p < cap; ++p) {
            bool real;
            uint64_t row;
            uint32_t slot;
            if (!bloom_host_entry(b, ks, cap, rows, count, slots, q, p, &real, &row, &slot)) continue;
            uint8_t* bits = b.bits + (size_t)slot * bloom_bytes(b.m);
            const uint8_t* d = ks.bytes + ks.offsets[row];
            const size_t len = ks.offsets[row + 1] - ks.offsets[row];
            for (uint32_t j = 0; j < b.k; ++j) {
                const uint32_t loc = bloom_location(d, len, b.seeds[j], b.m);
                bits[bloom_byte_of(loc)] |= bloom_mask_of(loc);
            }
        }
}
// the filter's decision: keep [nq][cap], 1 for the real entries whose Exists is false (user_item_exposure_bloom_filter.go:92-98)
inline void bloom_keep_host(const BloomHost& b, const BloomKeysHost& ks, uint32_t nq, uint32_t cap, const uint64_t* rows, const uint32_t* count,
                            const uint32_t* slots, uint8_t* keep) {
    for (uint32_t q = 0; q < nq; ++q)
        for (uint32_t p = 0; p < cap; ++p) {
            bool real;
            uint64_t row;
            uint32_t slot;
            const bool probe = bloom_host_entry(b, ks, cap, rows, count, slots, q, p, &real, &row, &slot);
            keep[(size_t)q * cap + p] = real && !(probe && bloom_host_test(b, ks, row, slot)) ? 1 : 0;
        }
}
// a slot's write as the device does it: n <= bloom_bytes(m) Redis bytes, the rest of the slot zero, the bits at or above m cleared
inline void bloom_slot_write_host(uint32_t m, uint8_t* slot_bits, const uint8_t* bytes, uint64_t n) {
    const uint64_t nb = bloom_bytes(m);
    if (n) memcpy(slot_bits, bytes, n);
    memset(slot_bits + n, 0, nb - n);
    slot_bits[nb - 1] &= bloom_last_byte_mask(m);
}

}  // namespace pg
