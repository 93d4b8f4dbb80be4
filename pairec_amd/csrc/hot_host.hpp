// hot_host.hpp — what a list recall's answer IS (UserGroupHotRecall, UserGlobalHotRecall, UserTopicRecall: DESIGN.md 4.1aa),
// free of HIP: the limits, the validation of an uploaded pg_hottable, the argument checks and the sizing of every request, the
// topic quotas, the keyed draw, the sort key, and the host statement the device kernel reproduces bit for bit.  hot.hip includes
// it for both sides; tests/hot_check.cpp builds it with a host compiler alone.
//
// The reference: module/user_group_hot_recall_hologres_dao.go:47-140 concatenates the item_ids rows of the user's trigger ids
// (entries "id", "id:source", "id:source:score"), sorts by score descending and cuts to RecallCount;
// module/user_global_hot_recall_hologres_dao.go:50-149 reads one list, gives an entry without a score rand.Float64() and sorts
// and cuts only a list longer than RecallCount; module/user_topic_mysql_dao.go:58-138 gives each topic of the user
// int(value / total * RecallCount) places and concatenates the heads of the topics' article lists in stored order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/pairec_gpu.h"

#ifdef __HIPCC__
#define PG_HOT_HD __host__ __device__ __forceinline__
#else
#define PG_HOT_HD inline
#endif

namespace pg {

constexpr uint32_t kHotMaxEntries = 65536;       // entries of one stored list, and of one request's concatenation
constexpr uint32_t kHotMaxQueries = 256, kHotMaxTriggers = 256, kHotMaxK = 16384;
constexpr uint32_t kHotLdsRecords = 8192;        // a request whose padded entry count is at most this orders in LDS
constexpr uint64_t kHotMaxPairs = 1ull << 40;    // a sort record keeps an entry's index in 40 bits
constexpr uint8_t kHotUnscored = 0x80, kHotSourceMask = 0x7F, kHotPadSource = 0xFF;
constexpr uint32_t kHotNone = 0xFFFFFFFFu;
static_assert(kHotMaxEntries == PG_HOT_MAX_ENTRIES && kHotUnscored == PG_HOT_UNSCORED && kHotPadSource == PG_HOT_PAD_SOURCE,
              "include/pairec_gpu.h states these for the callers");

// ---- the pieces both sides run ---------------------------------------------------------------------------------------------------
// u(q, p) of an unscored entry in PG_HOT_GLOBAL: pg_mix_sort's draw (the splitmix64 finaliser) of seed + golden * (1 + p), its
// top 53 bits as a double in [0, 1)
PG_HOT_HD double hot_draw(unsigned long long seed, uint32_t p) {
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * (1ull + (unsigned long long)p);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * 1.1102230246251565404236316680908203125e-16;      // 2^-53: both steps are exact
}
// the score's bits mapped so that ascending keys are descending scores, -0.0 ranking as 0.0 (cf_kernel.hpp's cf_finish)
PG_HOT_HD unsigned long long hot_key(unsigned long long score_bits) {
    unsigned long long b = score_bits;
    if (b == 0x8000000000000000ull) b = 0;
    const unsigned long long asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~asc;
}
PG_HOT_HD unsigned long long hot_bits(double v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (unsigned long long)__double_as_longlong(v);
#else
    unsigned long long b;
    memcpy(&b, &v, 8);
    return b;
#endif
}
// the score of the entry at position p: stored, or what an entry without one gets in `mode`
PG_HOT_HD double hot_entry_score(int mode, uint8_t source, double stored, unsigned long long seed, uint32_t p) {
    if (!(source & kHotUnscored)) return stored;
    return mode == PG_HOT_GLOBAL ? hot_draw(seed, p) : 0.0;
}

// ---- refusals: a code and a message, for callers with their own error convention ------------------------------------------------
struct HotRefusal {
    int code = PG_OK;
    char msg[256] = {0};
};
#define PG_HOT_REFUSE(r, c, ...)                              \
    do {                                                      \
        (r)->code = (c);                                      \
        snprintf((r)->msg, sizeof (r)->msg, __VA_ARGS__);     \
        return false;                                         \
    } while (0)

// ---- uploads -----------------------------------------------------------------------------------------------------------------------
// The lists of `n` consecutive triggers from `first` arrive as CSR: list i is entries [offsets[i], offsets[i + 1]) of item_rows /
// scores / source.  false for offsets that descend, a list longer than kHotMaxEntries, a row >= rows, a non-finite score, a
// source of 0xFF, an entry marked unscored that carries a score other than 0, or a table that would reach 2^40 entries.  A row
// twice in a list is allowed.  Nothing is read outside [offsets[0], offsets[n]), and only once every offset is known to ascend.
inline bool hot_validate_lists(const char* who, uint64_t first, uint64_t n, const uint64_t* offsets, const uint32_t* item_rows,
                               const double* scores, const uint8_t* source, uint64_t rows, uint64_t pairs_before, HotRefusal* r) {
    if (!offsets) PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: NULL argument", who);
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i])
            PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: offsets[%llu] is below offsets[%llu]", who, (unsigned long long)(i + 1), (unsigned long long)i);
        if (offsets[i + 1] - offsets[i] > kHotMaxEntries)
            PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: the list of trigger %llu has %llu entries (at most %u)", who, (unsigned long long)(first + i),
                          (unsigned long long)(offsets[i + 1] - offsets[i]), kHotMaxEntries);
    }
    const uint64_t total = n ? offsets[n] - offsets[0] : 0;
    if (total && !(item_rows && scores && source)) PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: NULL argument", who);
    if (total >= kHotMaxPairs || pairs_before >= kHotMaxPairs - total)
        PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: %llu entries behind the table's %llu (fewer than 2^40 in all)", who, (unsigned long long)total,
                      (unsigned long long)pairs_before);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t e = offsets[i]; e < offsets[i + 1]; ++e) {
            const unsigned long long t = first + i, at = e - offsets[i];
            if (item_rows[e] >= rows)
                PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: item row %u (entry %llu of trigger %llu) is outside the table's %llu rows", who, item_rows[e], at,
                              t, (unsigned long long)rows);
            if (!std::isfinite(scores[e])) PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: the score of entry %llu of trigger %llu is not finite", who, at, t);
            if (source[e] == kHotPadSource)
                PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: the source of entry %llu of trigger %llu is 0xFF (the output padding)", who, at, t);
            if ((source[e] & kHotUnscored) && scores[e] != 0.0)
                PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: entry %llu of trigger %llu is marked unscored and carries the score %g (must be 0)", who, at, t,
                              scores[e]);
        }
    return true;
}

// ---- arguments ---------------------------------------------------------------------------------------------------------------------
// The checks every form of the recall makes, in this order.
inline bool hot_check_args(const char* who, int mode, const uint32_t* triggers, const double* values, const uint32_t* off, uint32_t nq, uint32_t k,
                           const void* out_rows, const void* out_scores, HotRefusal* r) {
    if (!off || !out_rows || !out_scores) PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: NULL argument", who);
    if (mode != PG_HOT_GROUP && mode != PG_HOT_GLOBAL && mode != PG_HOT_TOPIC)
        PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: mode %d (PG_HOT_GROUP, PG_HOT_GLOBAL or PG_HOT_TOPIC)", who, mode);
    if (nq < 1 || nq > kHotMaxQueries) PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: nq=%u must be in [1,%u]", who, nq, kHotMaxQueries);
    if (k < 1 || k > kHotMaxK) PG_HOT_REFUSE(r, PG_ERR_UNSUPPORTED, "%s: k=%u unsupported (1..%u)", who, k, kHotMaxK);
    for (uint32_t q = 0; q < nq; ++q) {
        if (off[q + 1] < off[q])
            PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: trigger_offsets[%u] = %u is below trigger_offsets[%u] = %u", who, q + 1, off[q + 1], q, off[q]);
        if (off[q + 1] - off[q] > kHotMaxTriggers)
            PG_HOT_REFUSE(r, PG_ERR_UNSUPPORTED, "%s: request %u has %u triggers (at most %u per request)", who, q, off[q + 1] - off[q],
                          kHotMaxTriggers);
    }
    if (off[nq] != off[0] && (!triggers || (mode == PG_HOT_TOPIC && !values))) PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: NULL argument", who);
    if (mode == PG_HOT_TOPIC)
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = off[q]; i < off[q + 1]; ++i)
                if (!(std::isfinite(values[i]) && values[i] >= 0.0))
                    PG_HOT_REFUSE(r, PG_ERR_INVALID, "%s: trigger_value of trigger %u of request %u is %g (finite and >= 0)", who, i - off[q], q,
                                  values[i]);
    return true;
}

// UserTopicRecall's places (user_topic_mysql_dao.go:75-77, :101-106): v_j = value, 0 taken as 0.5; total = their sum in trigger
// order; take_j = (int64)((v_j / total) * (double)k), cut to what a uint32 holds.  Values are finite and >= 0 (hot_check_args):
// total is positive, or +inf when the sum overflows — then every share is 0.
inline void hot_topic_quotas(const double* values, uint32_t nt, uint32_t k, uint32_t* quota) {
    double total = 0.0;
    for (uint32_t j = 0; j < nt; ++j) total = total + (values[j] == 0.0 ? 0.5 : values[j]);
    for (uint32_t j = 0; j < nt; ++j) {
        const double v = values[j] == 0.0 ? 0.5 : values[j];
        const double share = (v / total) * (double)k;                        // <= k, never NaN: 0 < v <= total
        const long long take = (long long)share;
        quota[j] = (uint32_t)std::min<long long>(std::max<long long>(take, 0), 0xFFFFFFFFll);
    }
}

// What each trigger of one request contributes: len[j] = the entries of trigger j's list that enter the concatenation (the whole
// list; in PG_HOT_TOPIC its first min(take_j, len_j); nothing for a trigger of UINT32_MAX or >= n_triggers), quota[j] = take_j
// (PG_HOT_TOPIC only, else UINT32_MAX).  Returns n, their sum.  offsets: the table's [n_triggers + 1].
inline uint64_t hot_request_plan(int mode, uint32_t n_triggers, const uint64_t* offsets, const uint32_t* triggers, const double* values,
                                 uint32_t nt, uint32_t k, uint32_t* quota, uint32_t* len) {
    if (mode == PG_HOT_TOPIC) hot_topic_quotas(values, nt, k, quota);
    uint64_t n = 0;
    for (uint32_t j = 0; j < nt; ++j) {
        if (mode != PG_HOT_TOPIC) quota[j] = 0xFFFFFFFFu;
        const uint32_t t = triggers[j];
        uint64_t l = t < n_triggers ? offsets[t + 1] - offsets[t] : 0;
        l = std::min<uint64_t>(l, quota[j]);
        len[j] = (uint32_t)l;                                                // (a stored list holds at most kHotMaxEntries)
        n += l;
    }
    return n;
}
// is the answer of a request of n entries ordered by score?
PG_HOT_HD bool hot_is_sorted(int mode, uint64_t n, uint32_t k) { return mode == PG_HOT_GROUP || (mode == PG_HOT_GLOBAL && n > k); }
PG_HOT_HD uint32_t hot_next_pow2(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
// the refusal of a batch whose request q holds n > kHotMaxEntries entries
inline bool hot_refuse_size(const char* who, uint32_t q, uint64_t n, HotRefusal* r) {
    PG_HOT_REFUSE(r, PG_ERR_UNSUPPORTED, "%s: request %u concatenates %llu entries (at most %u per request)", who, q, (unsigned long long)n,
                  kHotMaxEntries);
}

// What a device call stages for its kernel, as ONE array of words in this order: [nq + 1] trigger offsets from 0, [nq] every
// request's n, [nq] its first record in the scratch slab (kHotNone: it orders in LDS, or not at all), [total] trigger ids,
// [total] quotas (PG_HOT_TOPIC only).  slab_records: the records the scratch-tier requests need, each its padded count.
struct HotStage {
    std::vector<uint32_t> words;
    size_t n_at = 0, slab_at = 0, trig_at = 0, quota_at = 0;     // where the regions behind the offsets start
    size_t slab_records = 0;
};
// Sizes every request of a checked batch from the table's offsets and fills *st.  false: the smallest request beyond
// kHotMaxEntries is refused in *r.
inline bool hot_stage_build(const char* who, int mode, uint32_t n_triggers, const uint64_t* offsets, const uint32_t* triggers,
                            const double* values, const uint32_t* off, uint32_t nq, uint32_t k, HotStage* st, HotRefusal* r) {
    const uint32_t total = off[nq] - off[0];
    const bool topic = mode == PG_HOT_TOPIC;
    st->n_at = (size_t)nq + 1;
    st->slab_at = st->n_at + nq;
    st->trig_at = st->slab_at + nq;
    st->quota_at = st->trig_at + total;
    st->words.assign(st->quota_at + (topic ? total : 0), 0u);
    st->slab_records = 0;
    uint32_t quota[kHotMaxTriggers], len[kHotMaxTriggers];
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t b = off[q] - off[0], nt = off[q + 1] - off[q];
        const uint64_t n = hot_request_plan(mode, n_triggers, offsets, nt ? triggers + off[q] : nullptr, topic && nt ? values + off[q] : nullptr,
                                            nt, k, quota, len);
        if (n > kHotMaxEntries) return hot_refuse_size(who, q, n, r);
        st->words.at(q) = b;
        st->words.at(st->n_at + q) = (uint32_t)n;
        st->words.at(st->slab_at + q) = kHotNone;
        const uint32_t np2 = hot_next_pow2((uint32_t)n);
        if (hot_is_sorted(mode, n, k) && np2 > kHotLdsRecords) {
            st->words.at(st->slab_at + q) = (uint32_t)st->slab_records;
            st->slab_records += np2;
        }
        for (uint32_t j = 0; j < nt; ++j) {
            st->words.at(st->trig_at + b + j) = triggers[off[q] + j];
            if (topic) st->words.at(st->quota_at + b + j) = quota[j];
        }
    }
    st->words.at(nq) = total;
    return true;
}

// ---- the host statement ----------------------------------------------------------------------------------------------------------
struct HotTableHost {
    uint64_t rows, row_offset;
    uint32_t n_triggers;
    const uint64_t* offsets;             // [n_triggers + 1], indexing the three arrays as they stand
    const uint32_t* item_rows;
    const double* scores;
    const uint8_t* source;
};
// The answer of nq requests (arguments checked by hot_check_args, the table by hot_validate_lists).  false: the smallest request
// beyond kHotMaxEntries is refused in *r and nothing is written.  seed: [nq] or NULL = 0; out_source / out_count optional.
inline bool hot_recall_host(const char* who, const HotTableHost& t, int mode, const uint32_t* triggers, const double* values, const uint32_t* off,
                            const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows, double* out_scores, uint8_t* out_source,
                            uint32_t* out_count, HotRefusal* r) {
    uint32_t quota[kHotMaxTriggers], len[kHotMaxTriggers];
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t n = hot_request_plan(mode, t.n_triggers, t.offsets, triggers + off[q], mode == PG_HOT_TOPIC ? values + off[q] : nullptr,
                                            off[q + 1] - off[q], k, quota, len);
        if (n > kHotMaxEntries) return hot_refuse_size(who, q, n, r);
    }
    std::vector<std::pair<unsigned long long, unsigned long long>> rec;          // (key, p << 40 | entry)
    std::vector<uint64_t> entry;                                                 // position p -> entry index
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t nt = off[q + 1] - off[q];
        const uint32_t* tg = triggers + off[q];
        const uint64_t n = hot_request_plan(mode, t.n_triggers, t.offsets, tg, mode == PG_HOT_TOPIC ? values + off[q] : nullptr, nt, k, quota, len);
        const unsigned long long sd = seed ? seed[q] : 0ull;
        entry.clear();
        for (uint32_t j = 0; j < nt; ++j)
            for (uint32_t i = 0; i < len[j]; ++i) entry.push_back(t.offsets[tg[j]] + i);
        if (hot_is_sorted(mode, n, k)) {
            rec.clear();
            for (uint32_t p = 0; p < n; ++p) {
                const uint64_t e = entry[p];
                rec.emplace_back(hot_key(hot_bits(hot_entry_score(mode, t.source[e], t.scores[e], sd, p))), ((unsigned long long)p << 40) | e);
            }
            std::sort(rec.begin(), rec.end());
        }
        const uint32_t kept = (uint32_t)std::min<uint64_t>(n, k);
        for (uint32_t j = 0; j < k; ++j) {
            const size_t o = (size_t)q * k + j;
            if (j >= kept) {
                out_rows[o] = ~0ull;
                out_scores[o] = -__builtin_inf();
                if (out_source) out_source[o] = kHotPadSource;
                continue;
            }
            const uint32_t p = hot_is_sorted(mode, n, k) ? (uint32_t)(rec[j].second >> 40) : j;
            const uint64_t e = entry[p];
            out_rows[o] = t.row_offset + t.item_rows[e];
            out_scores[o] = hot_entry_score(mode, t.source[e], t.scores[e], sd, p);
            if (out_source) out_source[o] = t.source[e] & kHotSourceMask;
        }
        if (out_count) out_count[q] = kept;
    }
    return true;
}

}  // namespace pg
