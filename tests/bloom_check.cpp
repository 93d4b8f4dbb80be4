// bloom_check.cpp — csrc/bloom_host.hpp alone, built with a host compiler (tests/test_bloom_san_cpu.py: plain, and under the
// address and undefined-behaviour sanitizers): the public murmur3_x86_32 vectors; keys of every length 0 .. 64 through the
// packed-word path the kernels take against the byte path; the locations and Redis's bit addressing at m = 1, 7, 8, 9 and
// 2^32 - 1; the key store's validation on hostile offsets; EstimateParameters; and the host statements on a grid of lists
// (padding, rows outside the store, users without a slot, slots past the end).
#include "bloom_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <random>

using namespace pg;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static uint32_t hash_packed(const BloomKeysPacked& pk, uint64_t row, uint32_t seed) {
    const uint64_t d = pk.desc[row];
    const uint32_t len = (uint32_t)(d & 0xFF);
    uint32_t mixed[kBloomKeyWords + 1] = {0};
    for (uint32_t i = 0; i < (len + 3) / 4; ++i) mixed[i] = bloom_mix(pk.words[(d >> 8) + i]);
    return bloom_hash_mixed(mixed, len, seed);
}

static void check_murmur() {
    struct { const char* key; uint32_t seed, want; } v[] = {
        {"", 0, 0}, {"", 1, 0x514E28B7u}, {"", 0xFFFFFFFFu, 0x81F16F39u}, {"test", 0, 0xBA6BD213u}, {"Hello, world!", 0, 0xC0363E43u},
        {"The quick brown fox jumps over the lazy dog", 0x9747B28Cu, 0x2FA826CDu}};
    for (const auto& x : v) CHECK(bloom_murmur3(reinterpret_cast<const uint8_t*>(x.key), strlen(x.key), x.seed) == x.want);
    // every length, from an odd address, through both paths
    std::mt19937 rng(7);
    std::vector<uint8_t> bytes(1);                                         // (keys start at offset 1: unaligned for the byte path)
    std::vector<uint64_t> off = {1};
    for (uint32_t len = 0; len <= kBloomMaxKey; ++len) {
        for (uint32_t i = 0; i < len; ++i) bytes.push_back((uint8_t)rng());
        off.push_back(bytes.size());
    }
    BloomRefusal r;
    CHECK(bloom_keys_validate(kBloomMaxKey + 1, off.data(), bytes.data(), "t", &r));
    BloomKeysPacked pk;
    bloom_keys_pack(kBloomMaxKey + 1, off.data(), bytes.data(), &pk);
    for (uint32_t len = 0; len <= kBloomMaxKey; ++len) {
        CHECK((pk.desc[len] & 0xFF) == len);
        for (uint32_t seed : {0u, 2u, 0xFFFFFFFFu, 0x9747B28Cu})
            CHECK(hash_packed(pk, len, seed) == bloom_murmur3(bytes.data() + off[len], len, seed));
    }
    // no keys at all: one word to point at
    BloomKeysPacked none;
    const uint64_t zero = 0;
    bloom_keys_pack(0, &zero, nullptr, &none);
    CHECK(none.desc.empty() && none.words.size() == 1);
    // decimal keys
    std::vector<uint64_t> doff;
    std::vector<uint8_t> dbytes;
    const int64_t ids[] = {0, -1, 10000000, INT64_MIN, INT64_MAX};
    bloom_keys_decimal(5, ids, &doff, &dbytes);
    const std::string all(dbytes.begin(), dbytes.end());
    CHECK(all == "0-110000000-92233720368547758089223372036854775807" && doff[5] == all.size() && doff[1] == 1 && doff[2] == 3);
}

static void check_bits() {
    CHECK(bloom_mask_of(0) == 0x80 && bloom_byte_of(0) == 0 && bloom_mask_of(7) == 0x01 && bloom_byte_of(8) == 1 && bloom_mask_of(8) == 0x80);
    CHECK(bloom_byte_of(0xFFFFFFFEu) == 0x1FFFFFFFu && bloom_mask_of(0xFFFFFFFEu) == 0x02);
    // the word view: byte b of a little-endian word holds bits 8 b .. 8 b + 7, most significant first
    for (uint32_t n = 0; n < 64; ++n) {
        uint8_t bytes[8] = {0};
        bytes[bloom_byte_of(n)] = bloom_mask_of(n);
        uint32_t w[2];
        memcpy(w, bytes, 8);
        CHECK(w[n >> 5] == bloom_word_bit(n) && w[1 - (n >> 5)] == 0);
    }
    CHECK(bloom_bytes(1) == 1 && bloom_bytes(8) == 1 && bloom_bytes(9) == 2 && bloom_bytes(0xFFFFFFFFu) == 0x20000000ull);
    CHECK(bloom_last_byte_mask(1) == 0x80 && bloom_last_byte_mask(7) == 0xFE && bloom_last_byte_mask(8) == 0xFF && bloom_last_byte_mask(9) == 0x80);
    CHECK(bloom_slot_stride(1) == 256 && bloom_slot_stride(2048) == 256 && bloom_slot_stride(2049) == 512 && bloom_slot_stride(0xFFFFFFFFu) == 0x20000000ull);
    for (uint32_t m : {1u, 7u, 8u, 9u, 2049u}) {                          // the last word of a slot lies inside its stride
        CHECK((uint64_t)((m - 1) >> 5) * 4 + 4 <= bloom_slot_stride(m));
        std::vector<uint8_t> slot(bloom_bytes(m), 0xAA), ones(bloom_bytes(m), 0xFF);
        bloom_slot_write_host(m, slot.data(), ones.data(), ones.size());
        CHECK(slot.back() == bloom_last_byte_mask(m));
        bloom_slot_write_host(m, slot.data(), nullptr, 0);
        for (uint8_t b : slot) CHECK(b == 0);
    }
    CHECK((uint64_t)((0xFFFFFFFFu - 1) >> 5) * 4 + 4 <= bloom_slot_stride(0xFFFFFFFFu));
}

static void check_validation() {
    BloomRefusal r;
    const uint8_t bytes[200] = {0};
    const uint64_t ok[] = {3, 3, 10, 74};
    CHECK(bloom_keys_validate(3, ok, bytes, "t", &r));
    CHECK(!bloom_keys_validate(3, nullptr, bytes, "t", &r) && r.code == PG_ERR_INVALID);
    const uint64_t down[] = {0, 5, 3, 8};
    CHECK(!bloom_keys_validate(3, down, bytes, "t", &r) && r.code == PG_ERR_INVALID && strstr(r.msg, "row 1"));
    const uint64_t lng[] = {0, 64, 129};
    CHECK(!bloom_keys_validate(2, lng, bytes, "t", &r) && r.code == PG_ERR_UNSUPPORTED && strstr(r.msg, "65 bytes"));
    CHECK(bloom_keys_validate(1, lng, bytes, "t", &r));
    const uint64_t wrap[] = {~0ull - 1, 2};                                // descends although the difference wraps to 4
    CHECK(!bloom_keys_validate(1, wrap, bytes, "t", &r) && r.code == PG_ERR_INVALID);
    const uint64_t far[] = {0, ~0ull};
    CHECK(!bloom_keys_validate(1, far, bytes, "t", &r) && r.code == PG_ERR_UNSUPPORTED);
    CHECK(!bloom_keys_validate(3, ok, nullptr, "t", &r) && r.code == PG_ERR_INVALID);
    const uint64_t empty[] = {9, 9, 9};
    CHECK(bloom_keys_validate(2, empty, nullptr, "t", &r));                // nothing to read: no bytes needed
    CHECK(bloom_keys_validate(0, empty, nullptr, "t", &r));
    CHECK(!bloom_check_params(0, 4, "t", &r) && !bloom_check_params(1ull << 32, 4, "t", &r) && bloom_check_params(0xFFFFFFFFull, 16, "t", &r));
    CHECK(!bloom_check_params(8, 0, "t", &r) && !bloom_check_params(8, 17, "t", &r) && bloom_check_params(1, 1, "t", &r));
    CHECK(!bloom_check_slot(2, 2, 0, 8, "t", &r) && bloom_check_slot(1, 2, 1, 8, "t", &r) && !bloom_check_slot(1, 2, 2, 8, "t", &r));
    uint64_t m;
    uint32_t k;
    CHECK(bloom_estimate(1000000, 0.05, &m, &k) && m == 6235225 && k == 4);
    CHECK(bloom_estimate(4096, 0.01, &m, &k) && m == 39261 && k == 7);
    CHECK(bloom_estimate(3000, 0.05, &m, &k) && m == 18706 && k == 4);
    CHECK(!bloom_estimate(0, 0.05, &m, &k) && !bloom_estimate(5, 0.0, &m, &k) && !bloom_estimate(5, 1.0, &m, &k) && !bloom_estimate(5, NAN, &m, &k));
}

// the host statements on lists with every kind of entry, at one m
static void check_lists(uint32_t m, uint32_t k, const uint32_t* seeds, uint32_t nq, uint32_t cap) {
    std::mt19937_64 rng(m * 31ull + k);
    const uint64_t key_rows = 90;
    std::vector<uint64_t> off = {0};
    std::vector<uint8_t> bytes;
    for (uint64_t i = 0; i < key_rows; ++i) {
        const uint32_t len = i <= kBloomMaxKey ? (uint32_t)i : (uint32_t)(rng() % (kBloomMaxKey + 1));
        for (uint32_t j = 0; j < len; ++j) bytes.push_back((uint8_t)rng());
        off.push_back(bytes.size());
    }
    const uint32_t n_slots = 3;
    const uint64_t nb = bloom_bytes(m);
    uint8_t* bits = static_cast<uint8_t*>(calloc(n_slots * nb, 1));       // (2^32 - 1 bits: 3 x 512 MiB, touched where bits are set)
    if (!bits) {
        printf("FAIL: no memory for m=%u\n", m);
        ++g_fail;
        return;
    }
    BloomHost b{m, k, n_slots, {0}, bits};
    bloom_seeds(seeds, k, b.seeds);
    const BloomKeysHost ks{key_rows, off.data(), bytes.data()};
    std::vector<uint64_t> rows((size_t)nq * cap), add_rows((size_t)nq * cap);
    for (auto* v : {&rows, &add_rows})
        for (auto& r : *v) {
            const uint64_t x = rng() % 100;
            r = x < 5 ? kBloomPadRow : x < 10 ? key_rows + x : x < 12 ? (1ull << 40) : rng() % key_rows;
        }
    std::vector<uint32_t> count(nq), slots(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        count[q] = q % 3 == 0 ? cap + 2 : (uint32_t)(rng() % (cap + 1));
        const uint32_t pat[] = {1, kBloomNoSlot, 1, n_slots, n_slots + 7};
        slots[q] = pat[q % 5];
    }
    bloom_add_host(b, ks, nq, cap, add_rows.data(), count.data(), slots.data());
    // only slot 1 was written, and only below m
    for (uint64_t i : {(uint64_t)0, nb - 1}) CHECK(bits[i] == 0 && bits[2 * nb + i] == 0);
    CHECK((bits[nb + nb - 1] & (uint8_t)~bloom_last_byte_mask(m)) == 0);
    std::vector<uint8_t> ex((size_t)nq * cap), keep((size_t)nq * cap), ex_add((size_t)nq * cap);
    bloom_exists_host(b, ks, nq, cap, rows.data(), count.data(), slots.data(), ex.data());
    bloom_keep_host(b, ks, nq, cap, rows.data(), count.data(), slots.data(), keep.data());
    bloom_exists_host(b, ks, nq, cap, add_rows.data(), count.data(), slots.data(), ex_add.data());
    for (uint32_t q = 0; q < nq; ++q)
        for (uint32_t p = 0; p < cap; ++p) {
            const size_t i = (size_t)q * cap + p;
            const bool real = p < std::min(count[q], cap) && rows[i] != kBloomPadRow;
            const bool can = real && rows[i] < key_rows && slots[q] < n_slots;
            CHECK(keep[i] == (real && !ex[i]));
            if (!can) CHECK(ex[i] == 0);
            if (m == 1) CHECK(ex[i] == (can ? 1 : 0));                    // every location is bit 0, and bit 0 is set
            const bool added = p < std::min(count[q], cap) && add_rows[i] < key_rows && slots[q] < n_slots;
            CHECK(ex_add[i] == (added ? 1 : 0));                           // what was added is found; nothing else of that list can be
        }
    // without counts every position is a candidate
    bloom_exists_host(b, ks, nq, cap, add_rows.data(), nullptr, slots.data(), ex_add.data());
    free(bits);
}

int main() {
    check_murmur();
    check_bits();
    check_validation();
    const uint32_t seeds[kBloomMaxK] = {0, 0xFFFFFFFFu, 2, 0x9747B28Cu, 1, 0x80000000u, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41};
    for (uint32_t m : {1u, 7u, 8u, 9u, 31u, 32u, 33u, 2048u, 2049u, 18706u, 0xFFFFFFFFu}) {
        check_lists(m, 4, nullptr, 5, 70);
        check_lists(m, 16, seeds, 3, 257);
        check_lists(m, 1, seeds, 1, 1);
    }
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("bloom OK\n");
    return 0;
}
