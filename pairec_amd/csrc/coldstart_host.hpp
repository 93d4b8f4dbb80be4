// coldstart_host.hpp — what a ColdStartRecall answer IS, free of HIP: the OrderBy parser, the order-preserving
// key of a column value, the keyed permutation of the random order and the host statement the device kernels reproduce bit for
// bit.  coldstart.hip includes it for both sides; tests/coldstart_check.cpp builds it with a host compiler alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/pairec_gpu.h"

#ifdef __HIPCC__
#define PG_COLD_HD __host__ __device__ __forceinline__
#else
#define PG_COLD_HD inline
#endif

namespace pg {

constexpr uint32_t kColdRounds = 8;        // Feistel rounds of the permutation (4 fail the pair tests on small pools)
constexpr uint32_t kColdMaxK = 16384, kColdMaxQueries = 256;
enum ColdOrder : int { kColdRandom = 0, kColdAsc = 1, kColdDesc = 2 };

struct ColdSpec {
    int order = kColdRandom;
    std::string column;                    // empty for the random order
};

// ---- OrderBy -----------------------------------------------------------------------------------------------------------
//   order_by := ws* ( "random" ws* "(" ws* ")" | column ( ws+ ( "ASC" | "DESC" ) )? )? ws*
// keywords in any case, column [A-Za-z_][A-Za-z0-9_]*.  NULL and "" are the random order.  false: *err_pos is the byte position
// of the first thing the grammar does not take and *err_msg says what was expected there.
inline bool cold_parse_order(const char* s, ColdSpec* out, size_t* err_pos, const char** err_msg) {
    out->order = kColdRandom;
    out->column.clear();
    if (!s) return true;
    const size_t n = strlen(s);
    size_t pos = 0;
    auto ws = [&] { while (pos < n && (s[pos] == ' ' || s[pos] == '\t' || s[pos] == '\n' || s[pos] == '\r')) ++pos; };
    auto alpha = [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; };
    auto digit = [](char c) { return c >= '0' && c <= '9'; };
    auto fail = [&](size_t at, const char* msg) { *err_pos = at; *err_msg = msg; return false; };
    auto ident = [&](std::string* raw, std::string* lower) {
        size_t e = pos;
        while (e < n && (alpha(s[e]) || digit(s[e]))) ++e;
        raw->assign(s + pos, e - pos);
        *lower = *raw;
        for (char& ch : *lower) if (ch >= 'A' && ch <= 'Z') ch = (char)(ch - 'A' + 'a');
        pos = e;
    };
    ws();
    if (pos == n) return true;
    if (!alpha(s[pos])) return fail(pos, "expected a column name or random()");
    std::string raw, lower;
    ident(&raw, &lower);
    const size_t after = pos;
    ws();
    if (lower == "random" && pos < n && s[pos] == '(') {
        ++pos;
        ws();
        if (pos >= n || s[pos] != ')') return fail(pos, "expected ')' of random()");
        ++pos;
        ws();
        if (pos != n) return fail(pos, "unexpected text after random()");
        return true;
    }
    int order = kColdAsc;
    if (pos != n) {
        if (pos == after || !alpha(s[pos])) return fail(pos, "expected ASC, DESC or the end after the column (one column, no expression)");
        const size_t at = pos;
        std::string kraw, kw;
        ident(&kraw, &kw);
        if (kw == "desc") order = kColdDesc;
        else if (kw != "asc") return fail(at, "expected ASC or DESC after the column");
        ws();
        if (pos != n) return fail(pos, "unexpected text after the direction (one column, no NULLS FIRST / LAST)");
    }
    out->order = order;
    out->column = raw;
    return true;
}

// ---- keys --------------------------------------------------------------------------------------------------------------
// A column value as an unsigned key whose order is the column's.  Integers: the sign bit flipped.  Floats: -0.0 taken as +0.0,
// every NaN the one largest key (Postgres: NaN = NaN, NaN > every number), then the total-order transform of the bit pattern.
// An F32 key is that transform of its 32 bits in the high half of the word: the order of the exactly widened values, computed
// without a conversion instruction (whose treatment of subnormals depends on the float mode).
PG_COLD_HD uint64_t cold_key_i64(long long v) { return (uint64_t)v ^ 0x8000000000000000ull; }
PG_COLD_HD uint64_t cold_key_f64_bits(uint64_t b) {
    if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return ~0ull;
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
PG_COLD_HD uint64_t cold_key_f32_bits(uint32_t b) {
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return ~0ull;
    if (b == 0x80000000u) b = 0;
    const uint32_t k = (b >> 31) ? ~b : (b | 0x80000000u);
    return (uint64_t)k << 32;
}
// the key of row r of a column of `dtype` (PG_F_*); `desc` complements it, so that every order is "smallest key first"
// ... from the value's bit pattern `raw` (a 32-bit type's in the low half)
PG_COLD_HD uint64_t cold_key_raw(int dtype, uint64_t raw, bool desc) {
    uint64_t k;
    switch (dtype) {
        case PG_F_I32: k = cold_key_i64((long long)(int32_t)(uint32_t)raw); break;
        case PG_F_I64: k = cold_key_i64((long long)raw); break;
        case PG_F_F32: k = cold_key_f32_bits((uint32_t)raw); break;
        default: k = cold_key_f64_bits(raw); break;
    }
    return desc ? ~k : k;
}
PG_COLD_HD uint64_t cold_key_at(const void* col, int dtype, uint64_t r, bool desc) {
    const bool wide = dtype == PG_F_I64 || dtype == PG_F_F64;
    return cold_key_raw(dtype, wide ? reinterpret_cast<const uint64_t*>(col)[r] : (uint64_t)reinterpret_cast<const uint32_t*>(col)[r], desc);
}

// ---- the random order ----------------------------------------------------------------------------------------------------
// the splitmix64 finaliser (pg_mix_sort's draw uses the same)
PG_COLD_HD uint64_t cold_mix(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// h = b / 2 for the smallest even b >= 2 with 2^b >= A (A < 2^32: h <= 16)
PG_COLD_HD uint32_t cold_half_bits(uint64_t A) {
    uint32_t b = 2;
    while (b < 64 && (1ull << b) < A) b += 2;
    return b / 2;
}
// one application of the keyed bijection of [0, 2^(2h))
PG_COLD_HD uint64_t cold_perm_step(uint64_t seed, uint64_t x, uint32_t h) {
    const uint64_t mask = (1ull << h) - 1ull;
    uint64_t L = x >> h, R = x & mask;
    for (uint32_t r = 0; r < kColdRounds; ++r) {
        const uint64_t f = cold_mix(seed + 0x9E3779B97F4A7C15ull * (1ull + ((uint64_t)r << 32) + R)) & mask;
        const uint64_t nr = L ^ f;
        L = R;
        R = nr;
    }
    return (L << h) | R;
}
// P(i), i < A: cycle walking — a bijection of [0, 2^(2h)) restricted to [0, A) by re-applying it while it lands outside
PG_COLD_HD uint64_t cold_perm(uint64_t seed, uint64_t A, uint32_t h, uint64_t i) {
    uint64_t x = i;
    do x = cold_perm_step(seed, x, h); while (x >= A);
    return x;
}

// ---- the host statement ----------------------------------------------------------------------------------------------------
// bits: the clause's bitmap (bit r & 31 of word r >> 5), NULL = every row.  Outputs as every recall's: out_rows [nq][k] global
// ids then UINT64_MAX, out_scores [nq][k] 0.0f then -inf, out_count [nq] (optional) = min(k, A).  The arguments are the
// caller's to check (pg_cold_recall_host does).
inline void cold_recall_host(int order, const uint32_t* bits, uint64_t rows, uint64_t row_offset, const void* order_col, int order_dtype,
                             const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    std::vector<uint32_t> sel;
    for (uint64_t r = 0; r < rows; ++r)
        if (!bits || ((bits[r >> 5] >> (r & 31)) & 1u)) sel.push_back((uint32_t)r);
    const uint64_t A = sel.size();
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, A);
    const float ninf = -std::numeric_limits<float>::infinity();
    if (order != kColdRandom && kk) {
        const bool desc = order == kColdDesc;
        std::vector<uint64_t> key(A);
        for (uint64_t j = 0; j < A; ++j) key[j] = cold_key_at(order_col, order_dtype, sel[j], desc);
        std::vector<uint32_t> idx(A);
        for (uint64_t j = 0; j < A; ++j) idx[j] = (uint32_t)j;
        // (sel ascends, so the position in it breaks ties as the row does)
        std::partial_sort(idx.begin(), idx.begin() + kk, idx.end(),
                          [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
        for (uint32_t i = 0; i < kk; ++i) idx[i] = sel[idx[i]];
        sel.assign(idx.begin(), idx.begin() + kk);
    }
    const uint32_t h = cold_half_bits(A);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t s = seed ? seed[q] : 0;
        for (uint32_t i = 0; i < k; ++i) {
            const size_t o = (size_t)q * k + i;
            if (i < kk) {
                out_rows[o] = row_offset + (order == kColdRandom ? sel[cold_perm(s, A, h, i)] : sel[i]);
                out_scores[o] = 0.0f;
            } else {
                out_rows[o] = ~0ull;
                out_scores[o] = ninf;
            }
        }
        if (out_count) out_count[q] = kk;
    }
}

}  // namespace pg
