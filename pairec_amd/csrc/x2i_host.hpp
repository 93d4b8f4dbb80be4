// x2i_host.hpp — what a U2I2X2I answer IS, free of HIP: the limits, the validation of an uploaded side of a
// pg_xtable, the argument checks every form of the recall makes, and the host statement the device kernel reproduces bit for
// bit.  x2i.hip includes it for both sides; tests/x2i_check.cpp builds it with a host compiler alone.
//
// Reference: module/user_collaborative_u2i2x2i_hologres_dao.go:73-348 and module/realtime_user2item_u2i2x2i_hologres_dao.go:94-270
// — trigger items -> their X values (hop 1, xPreferScoreMap[x] += prefer) -> the items listed under each X (hop 2, the request's
// trigger items skipped), summed per item and normalised (mergeUserCollaborativeItemsResult) or the largest term kept (uniqItems).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/pairec_gpu.h"

namespace pg {

constexpr uint32_t kX2iMaxXPerItem = 64;     // an item's X list
constexpr uint32_t kX2iMaxList = 1024;       // an X's item list: one entry per lane of the kernel's workgroup
constexpr uint32_t kX2iMaxX = 1024;          // distinct X of one request; beyond it the request is reported, never cut
constexpr uint32_t kX2iMaxPairs = 65536;     // (X, item) pairs of one request's X lists; the same
constexpr uint32_t kX2iMaxQueries = 256, kX2iMaxTriggers = 256, kX2iMaxK = 16384, kX2iMaxExclude = 4096;
// the status word of a batch: UINT32_MAX, or for the smallest request beyond a limit 2 q + (0: distinct X, 1: pairs)
constexpr uint32_t kX2iNone = 0xFFFFFFFFu;

inline std::string x2i_fmt(const char* fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    return buf;
}

// ---- uploads -----------------------------------------------------------------------------------------------------------------
// One side of the table arrives as CSR: list i of `n` consecutive keys from `first` is ids[offsets[i] .. offsets[i + 1])
// (scores beside them, or NULL for the item -> X side).  false, with *err set, for offsets that descend, a list longer than
// max_len, an id >= id_limit, a non-finite score or an id twice in one list.  Nothing is read outside
// [offsets[0], offsets[n]) of ids / scores, and only once every offset is known to ascend.
inline bool x2i_validate_lists(const char* who, const char* key_name, const char* id_name, uint64_t first, uint64_t n, const uint64_t* offsets,
                               const uint32_t* ids, const float* scores, uint64_t max_len, uint64_t id_limit, std::string* err) {
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) {
            *err = std::string(who) + x2i_fmt(": offsets[%llu] is below offsets[%llu]", i + 1, i);
            return false;
        }
        if (offsets[i + 1] - offsets[i] > max_len) {
            *err = std::string(who) + ": the list of " + key_name +
                   x2i_fmt(" %llu has %llu entries (at most %llu)", first + i, offsets[i + 1] - offsets[i], max_len);
            return false;
        }
    }
    if (n && offsets[n] > offsets[0] && (!ids)) {
        *err = std::string(who) + ": NULL argument";
        return false;
    }
    std::vector<uint32_t> seen;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b = offsets[i], len = offsets[i + 1] - b;
        for (uint64_t j = 0; j < len; ++j) {
            if (ids[b + j] >= id_limit) {
                *err = std::string(who) + ": " + id_name + x2i_fmt(" %llu in the list of ", ids[b + j]) + key_name +
                       x2i_fmt(" %llu is outside the table's %llu", first + i, id_limit);
                return false;
            }
            if (scores && !std::isfinite(scores[b + j])) {
                *err = std::string(who) + ": a score in the list of " + key_name + x2i_fmt(" %llu is not finite", first + i);
                return false;
            }
        }
        seen.assign(ids + b, ids + b + len);
        std::sort(seen.begin(), seen.end());
        for (uint64_t j = 1; j < len; ++j)
            if (seen[j] == seen[j - 1]) {
                *err = std::string(who) + ": " + id_name + x2i_fmt(" %llu appears twice in the list of ", seen[j]) + key_name +
                       x2i_fmt(" %llu", first + i);
                return false;
            }
    }
    return true;
}

// ---- arguments -----------------------------------------------------------------------------------------------------------------
// The checks every form of the recall makes, in this order.  PG_OK, or the error code with *err set.  dev_trig: the triggers are
// made by the call itself (pg_rtu2i_x_recall) — no trigger arrays, no offsets.  host_pref: trigger_prefer is host memory and is
// checked to be finite.  *nmax_out = the longest exclusion list.
inline int x2i_check_args(const char* who, const void* trig, const double* pref, const uint32_t* off, uint32_t nq, uint32_t k,
                          const pg_x2i_opts* opts, const void* rows, const void* scores, bool dev_trig, bool host_pref, uint32_t* nmax_out,
                          std::string* err) {
    const std::string w = who;
    if (!(off || dev_trig) || !rows || !scores) { *err = w + ": NULL argument"; return PG_ERR_INVALID; }
    if (nq < 1 || nq > kX2iMaxQueries) { *err = w + x2i_fmt(": nq=%llu must be in [1,%llu]", nq, kX2iMaxQueries); return PG_ERR_INVALID; }
    if (k < 1 || k > kX2iMaxK) { *err = w + x2i_fmt(": k=%llu unsupported (1..%llu)", k, kX2iMaxK); return PG_ERR_UNSUPPORTED; }
    for (uint32_t q = 0; q < nq && !dev_trig; ++q) {
        if (off[q + 1] < off[q]) {
            *err = w + x2i_fmt(": trigger_offsets[%llu] = %llu is below", q + 1, off[q + 1]) + x2i_fmt(" trigger_offsets[%llu] = %llu", q, off[q]);
            return PG_ERR_INVALID;
        }
        if (off[q + 1] - off[q] > kX2iMaxTriggers) {
            *err = w + x2i_fmt(": request %llu has %llu triggers (at most %llu per request)", q, off[q + 1] - off[q], kX2iMaxTriggers);
            return PG_ERR_UNSUPPORTED;
        }
    }
    if (!dev_trig && !(trig && pref) && off[nq] != off[0]) { *err = w + ": NULL argument"; return PG_ERR_INVALID; }
    if (!dev_trig && host_pref)
        for (uint32_t i = off[0]; i < off[nq]; ++i)
            if (!std::isfinite(pref[i])) { *err = w + x2i_fmt(": trigger_prefer[%llu] is not finite", i); return PG_ERR_INVALID; }
    uint32_t nmax = 0;
    const uint32_t* xo = opts ? opts->excl_offsets : nullptr;
    if (xo) {
        for (uint32_t q = 0; q < nq; ++q) {
            if (xo[q + 1] < xo[q]) {
                *err = w + x2i_fmt(": excl_offsets[%llu] = %llu is below", q + 1, xo[q + 1]) + x2i_fmt(" excl_offsets[%llu] = %llu", q, xo[q]);
                return PG_ERR_INVALID;
            }
            if (xo[q + 1] - xo[q] > kX2iMaxExclude) {
                *err = w + x2i_fmt(": request %llu excludes %llu ids (at most %llu per request)", q, xo[q + 1] - xo[q], kX2iMaxExclude);
                return PG_ERR_UNSUPPORTED;
            }
            nmax = std::max(nmax, xo[q + 1] - xo[q]);
        }
        if (!opts->excl_rows && xo[nq] != xo[0]) { *err = w + ": excl_rows is NULL"; return PG_ERR_INVALID; }
        if ((uint64_t)k + nmax > kX2iMaxK) {
            *err = w + x2i_fmt(": k=%llu plus the longest exclusion list of %llu ids exceeds the depth of %llu", k, nmax, kX2iMaxK);
            return PG_ERR_UNSUPPORTED;
        }
    } else if (opts && opts->excl_rows) {
        *err = w + ": excl_rows without excl_offsets";
        return PG_ERR_INVALID;
    }
    *nmax_out = nmax;
    return PG_OK;
}

// what the status word of a batch says, for the error message
inline std::string x2i_limit_message(const char* who, uint32_t status) {
    if (status & 1u)
        return std::string(who) + x2i_fmt(": the X lists of request %llu hold more than %llu (X, item) pairs", status >> 1, kX2iMaxPairs);
    return std::string(who) + x2i_fmt(": request %llu reaches more than %llu distinct X", status >> 1, kX2iMaxX);
}

// ---- the host statement ------------------------------------------------------------------------------------------------------------
// the sort key of a score: ascending key = descending score, -0.0 ranked as 0.0 (the records cf_finish orders)
inline uint64_t x2i_order_key(double sc) {
    uint64_t b;
    memcpy(&b, &sc, 8);
    if (b == 0x8000000000000000ull) b = 0;
    const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~asc;
}

// The answer of nq requests over host CSR arrays (the arguments are the caller's to check: x2i_check_args, and CSR that
// x2i_validate_lists accepts).  Returns the batch's status word (kX2iNone: every request served); a request beyond a limit
// answers 0 like the device.  out_count may be NULL.
inline uint32_t x2i_recall_host(uint64_t rows, uint64_t row_offset, uint32_t n_x, const uint64_t* i2x_off, const uint32_t* i2x_ids,
                                const uint64_t* x2i_off, const uint32_t* x2i_rows, const float* x2i_scores, const uint32_t* trig,
                                const double* pref, const uint32_t* off, uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* out_rows,
                                double* out_scores, uint32_t* out_count) {
    const bool max_rule = opts && opts->max_rule;
    const bool normalize = !max_rule && (opts ? opts->normalize != 0 : true);
    const uint32_t* xo = opts ? opts->excl_offsets : nullptr;
    uint32_t status = kX2iNone;
    for (uint32_t q = 0; q < nq; ++q) {
        uint64_t* orow = out_rows + (size_t)q * k;
        double* osc = out_scores + (size_t)q * k;
        uint32_t kept = 0;
        auto pad = [&] {
            for (uint32_t j = kept; j < k; ++j) {
                orow[j] = ~0ull;
                osc[j] = -std::numeric_limits<double>::infinity();
            }
            if (out_count) out_count[q] = kept;
        };
        // hop 1: the request's X in order of first appearance, their preferences added in trigger order
        std::unordered_set<uint32_t> tset;
        std::vector<uint32_t> xs;
        std::vector<double> xpref;
        std::unordered_map<uint32_t, size_t> xpos;
        for (uint32_t i = off[q]; i < off[q + 1]; ++i) {
            const uint32_t r = trig[i];
            if (r == 0xFFFFFFFFu || r >= rows) continue;
            tset.insert(r);
            for (uint64_t e = i2x_off[r]; e < i2x_off[r + 1]; ++e) {
                const uint32_t x = i2x_ids[e];
                if (x >= n_x) continue;
                auto it = xpos.find(x);
                if (it == xpos.end()) {
                    xpos.emplace(x, xs.size());
                    xs.push_back(x);
                    xpref.push_back(pref[i]);
                } else {
                    xpref[it->second] = xpref[it->second] + pref[i];
                }
            }
        }
        if (xs.size() > kX2iMaxX) {
            status = std::min(status, q * 2u);
            pad();
            continue;
        }
        uint64_t pairs = 0;
        for (size_t j = 0; j < xs.size(); ++j)
            if (std::isfinite(xpref[j])) pairs += x2i_off[xs[j] + 1] - x2i_off[xs[j]];
        if (pairs > kX2iMaxPairs) {
            status = std::min(status, q * 2u + 1u);
            pad();
            continue;
        }
        // hop 2: the X in that order, their lists in stored order, the request's trigger items skipped
        std::vector<uint32_t> items;
        std::vector<double> score;
        std::unordered_map<uint32_t, size_t> ipos;
        for (size_t j = 0; j < xs.size(); ++j) {
            if (!std::isfinite(xpref[j])) continue;
            for (uint64_t e = x2i_off[xs[j]]; e < x2i_off[xs[j] + 1]; ++e) {
                const uint32_t it = x2i_rows[e];
                if (it >= rows || tset.count(it)) continue;
                const double term = xpref[j] * (double)x2i_scores[e];
                auto f = ipos.find(it);
                if (f == ipos.end()) {
                    ipos.emplace(it, items.size());
                    items.push_back(it);
                    score.push_back(term);
                } else if (!max_rule) {
                    score[f->second] = score[f->second] + term;
                } else if (term > score[f->second]) {
                    score[f->second] = term;
                }
            }
        }
        if (normalize) {
            double m = 0.0;
            for (double s : score)
                if (s > m) m = s;
            if (m > 0.0)
                for (double& s : score) s = s / m;
        }
        std::vector<std::pair<uint64_t, uint32_t>> order(items.size());
        for (size_t j = 0; j < items.size(); ++j) order[j] = {x2i_order_key(score[j]), items[j]};
        std::sort(order.begin(), order.end());
        std::unordered_set<uint64_t> seen;
        if (xo) seen.insert(opts->excl_rows + xo[q], opts->excl_rows + xo[q + 1]);
        for (size_t j = 0; j < order.size() && kept < k; ++j) {
            const uint64_t id = row_offset + order[j].second;
            if (xo && seen.count(id)) continue;
            orow[kept] = id;
            osc[kept] = score[ipos[order[j].second]];
            ++kept;
        }
        pad();
    }
    return status;
}

}  // namespace pg
