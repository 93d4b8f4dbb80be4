// dimcap.hip — the value cap: keep, in order, at most `limit` entries per value of one feature-store column.
//
// DimensionFieldUniqueFilter (filter/dimension_field_unique_filter.go:33-55) keeps the first item of each value of a property
// and every item whose property is "" (:41-42): limit = 1, PG_DIMCAP_NULL_KEEP.  One dimension of GroupWeightCountFilter's
// groupWeightDimensionFilter (filter/group_weight_count_filter.go:288-302) keeps the first sizeLimit items of each value, ""
// being the value "__DEFAULT__" (:293-295): limit = sizeLimit, PG_DIMCAP_NULL_VALUE.  Either way an entry is kept iff fewer than
// `limit` earlier entries of its value were kept, and since a dropped entry has `limit` kept ones before it, that is: iff it is
// among the first `limit` OCCURRENCES of its value in the request.  So the kernel needs each entry's occurrence index, capped at
// limit, and nothing else.
//
// One workgroup of 1 024 lanes per request walks cap in chunks of 1 024 positions.  Per chunk:
//   load     the lane's row, then the column's value at the row (both before anything uses them);
//   slot     the value's slot in an open-addressed table of full 64-bit keys with a count per slot, found or claimed by
//            compare-and-swap (no slot is ever freed, so a duplicate always finds its value's slot).  Two more counts stand
//            behind the table: one for the value that equals the empty-slot mark, one for null under PG_DIMCAP_NULL_VALUE;
//   rank     within its wave, a lane's peers — the lanes with its slot — by one ballot per bit of the slot index: rank = the
//            peers below it, group = all of them;
//   count    the waves of the chunk in turn (a barrier between two): a lane reads its slot's count, is kept iff count + rank <
//            limit, and the last peer stores min(count + group, limit).  Waves in position order, lanes in position order
//            within the wave: no atomic decides an order;
//   compact  kept entries move to the front by block_rank.hpp's chunk_rank + a running base, with everything carried
//            (cand_carry).
// Two tiers by cap alone: up to kDimcapLdsMaxCap the table is dynamic LDS (12 bytes per slot, 2 cap slots: 144 KiB at the
// boundary), above it the request's slice of kSlotDimcap, every access an agent-scope atomic as the fan-in's scratch tier.
#include "cand_lists.hpp"
#include "block_rank.hpp"

#include <unordered_map>

namespace pg {
namespace {

constexpr uint32_t kDimcapChunk = 1024, kDimcapWaves = kDimcapChunk / kWave;
constexpr uint32_t kDimcapLdsMaxCap = 6144;      // the tier boundary: 2 * 6144 slots * 12 B = 144 KiB of a workgroup's 160
constexpr uint32_t kDimcapMinSlots = 1024;       // slots = max(2 cap, this): load factor <= 0.5
static_assert(kDimcapLdsMaxCap == PG_DIMCAP_LDS_MAX_CAP && kDimcapChunk == PG_DIMCAP_CHUNK && kDimcapMinSlots == PG_DIMCAP_MIN_SLOTS,
              "include/pairec_gpu.h repeats these");
static_assert((size_t)2 * kDimcapLdsMaxCap * 12 + 8 + 1024 <= 160 * 1024, "one workgroup's LDS (the wave counts are static LDS beside it)");
constexpr unsigned long long kDimcapEmpty = 0x8000000000000000ull;       // an empty slot; the value INT64_MIN counts behind the table

__host__ __device__ inline uint32_t dimcap_slots(uint32_t cap) { return 2 * cap > kDimcapMinSlots ? 2 * cap : kDimcapMinSlots; }
// the slot a key's probe starts at: the high half of key * 0x9E3779B97F4A7C15 scaled to [0, slots)  (the header states it:
// tests build colliding keys from it)
__host__ __device__ inline uint32_t dimcap_slot(unsigned long long key, uint32_t slots) {
    return (uint32_t)((((key * 0x9E3779B97F4A7C15ull) >> 32) * (unsigned long long)slots) >> 32);
}

struct DimcapArgs {
    CandIn in;
    CandOut out;                                 // (out_cap = cap)
    const void* col;                             // [store_rows] int32 or int64
    unsigned long long store_rows;
    long long null_value;
    uint32_t is_i64, limit, null_as_value, has_null;
    uint32_t slots;
    unsigned long long* gkeys;                   // scratch tier: [nq][slots]
    uint32_t* gcnt;                              // [nq][slots + 2]
};

// Request q = blockIdx.x.
template <bool kLds>
__global__ __launch_bounds__(kDimcapChunk) void dimcap_kernel(DimcapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dimcap_lds[];
    __shared__ uint32_t wcnt[2 * kDimcapWaves];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t slots = a.slots, limit = a.limit;
    unsigned long long* keys;
    uint32_t* cnt;                               // [slots + 2]: the table's, then the empty mark's value, then null
    if constexpr (kLds) {
        keys = reinterpret_cast<unsigned long long*>(dimcap_lds);
        cnt = reinterpret_cast<uint32_t*>(keys + slots);
    } else {
        keys = a.gkeys + (size_t)q * slots;
        cnt = a.gcnt + (size_t)q * (slots + 2);
    }
    for (uint32_t i = tid; i < slots + 2; i += kDimcapChunk) {
        if (i < slots) tab_store<kLds>(&keys[i], kDimcapEmpty);
        tab_store<kLds>(&cnt[i], 0u);
    }
    __syncthreads();
    uint32_t idx_bits = 0;                       // the bits of a slot index, the two behind the table included
    while (((slots + 1) >> idx_bits) != 0) ++idx_bits;
    const size_t q0 = (size_t)q * a.in.cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    uint32_t run = 0;                                                // the entries kept so far: every lane counts along
    for (uint32_t c0 = 0, it = 0; c0 < n_valid; c0 += kDimcapChunk, ++it) {
        const uint32_t pos = c0 + tid;
        bool keep = false, counted = false;
        uint32_t h = 0;
        if (pos < n_valid) {
            const unsigned long long row = a.in.rows[q0 + pos];
            if (row != kCandPad) {
                bool null = row >= a.store_rows;
                long long v = 0;
                if (!null) {
                    v = a.is_i64 ? reinterpret_cast<const long long*>(a.col)[row] : (long long)reinterpret_cast<const int32_t*>(a.col)[row];
                    null = a.has_null && v == a.null_value;
                }
                if (null) {
                    if (a.null_as_value) {
                        counted = true;
                        h = slots + 1;
                    } else {
                        keep = true;                                 // always kept, never counted
                    }
                } else {
                    counted = true;
                    const unsigned long long key = (unsigned long long)v;
                    if (key == kDimcapEmpty) {
                        h = slots;
                    } else {
                        for (h = dimcap_slot(key, slots);; h = h + 1 == slots ? 0 : h + 1) {
                            // (a read walks the occupied run, the compare-and-swap only claims a slot seen empty)
                            unsigned long long cur = tab_load<kLds>(&keys[h]);
                            if (cur == kDimcapEmpty) cur = atomicCAS(&keys[h], kDimcapEmpty, key);
                            if (cur == kDimcapEmpty || cur == key) break;
                        }
                    }
                }
            }
        }
        // rank: the lanes of this wave with the same slot
        unsigned long long peers = __ballot(counted);
        for (uint32_t b = 0; b < idx_bits; ++b) {
            const bool bit = (h >> b) & 1u;
            const unsigned long long m = __ballot(counted && bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull)), group = (uint32_t)__popcll(peers);
        // count: the waves in turn
        for (uint32_t w = 0; w < kDimcapWaves; ++w) {
            if (w == wave && counted) {
                const uint32_t have = tab_load<kLds>(&cnt[h]);     // (every peer reads before the last one stores: one instruction each)
                keep = (unsigned long long)have + rank < limit;
                const unsigned long long now = (unsigned long long)have + group;
                if (rank + 1 == group) tab_store<kLds>(&cnt[h], now < limit ? (uint32_t)now : limit);
            }
            __syncthreads();
        }
        // compact
        uint32_t r, total;
        chunk_rank<kDimcapWaves>(keep, wcnt, it, &r, &total);
        if (keep) cand_carry(a.in, a.out, q0 + pos, q0 + run + r, true);                   // (run + r <= pos < cap)
        run += total;
    }
    cand_pad(a.in, a.out, q, run + tid, kDimcapChunk, kCandNan);      // padding behind the count
    if (tid == 0) a.out.count[q] = run;
}

// what both device entries and the host statement check of a conf, after the NULL check
int dimcap_check_conf(const pg_dimcap_conf* conf, const char* who) {
    PG_REQUIRE(conf->limit >= 1, "%s: limit=0 keeps nothing (1 .. UINT32_MAX; 1 is DimensionFieldUniqueFilter)", who);
    PG_REQUIRE(conf->null_mode == PG_DIMCAP_NULL_KEEP || conf->null_mode == PG_DIMCAP_NULL_VALUE, "%s: unknown null_mode %u", who, conf->null_mode);
    return PG_OK;
}
int dimcap_check_cap(uint32_t cap, const char* who) {
    if (cap < 1 || cap > kCandMaxCap) {
        set_error("%s: cap=%u unsupported (1..%u)", who, cap, kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}

// the table of nq requests at cap: keys [nq][slots] | counts [nq][slots + 2]
size_t dimcap_table_bytes(uint32_t nq, uint32_t cap) {
    const size_t slots = dimcap_slots(cap);
    return align_up((size_t)nq * slots * 8) + (size_t)nq * (slots + 2) * 4;
}

// caller holds ctx->mu; one launch on the context's stream, no synchronisation.  table: dimcap_table_bytes of device memory for
// the scratch tier (NULL: kSlotDimcap is carved here)
int dimcap_locked(pg_ctx* ctx, const pg_features* fs, const pg_dimcap_conf* conf, const CandIn& in, const CandOut& out, void* table, const char* who) {
    // the column by name (cond_resolve_columns' messages)
    const pg_features::Column* col = nullptr;
    for (const auto& x : fs->cols)
        if (x.name == conf->column) { col = &x; break; }
    if (!col || !col->d) {
        set_error("%s: column \"%s\" is not a column of the feature store", who, conf->column);
        return PG_ERR_INVALID;
    }
    if (col->dtype != PG_F_I32 && col->dtype != PG_F_I64) {
        set_error("%s: column \"%s\" is a float column (dtype %d): the value cap serves int32 and int64 columns", who, conf->column, col->dtype);
        return PG_ERR_UNSUPPORTED;
    }
    DimcapArgs a{};
    a.in = in;
    a.out = out;
    a.col = col->d;
    a.store_rows = fs->rows;
    a.null_value = conf->null_value;
    a.is_i64 = col->dtype == PG_F_I64;
    a.limit = conf->limit;
    a.null_as_value = conf->null_mode == PG_DIMCAP_NULL_VALUE;
    a.has_null = conf->has_null != 0;
    a.slots = dimcap_slots(in.cap);
    int rc;
    if (in.cap <= kDimcapLdsMaxCap) {
        // (the limit is raised once, to the boundary's table; a launch asks for its own cap's)
        if ((rc = ensure_dyn_lds(ctx, (const void*)dimcap_kernel<true>, (size_t)dimcap_slots(kDimcapLdsMaxCap) * 12 + 8))) return rc;
        dimcap_kernel<true><<<in.nq, kDimcapChunk, (size_t)a.slots * 12 + 8, ctx->stream>>>(a);
    } else {
        char* t = (char*)table;
        if (!t && (rc = scratch_carve(ctx, kSlotDimcap, [&](Carve& c) { t = (char*)c.bytes(dimcap_table_bytes(in.nq, in.cap)); }))) return rc;
        a.gkeys = reinterpret_cast<unsigned long long*>(t);
        a.gcnt = reinterpret_cast<uint32_t*>(t + align_up((size_t)in.nq * a.slots * 8));
        dimcap_kernel<false><<<in.nq, kDimcapChunk, 0, ctx->stream>>>(a);
    }
    PG_HIP(hipGetLastError());
    return PG_OK;
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_candidates_dimcap_host(const pg_dimcap_conf* conf, uint32_t nq, uint32_t cap, const int64_t* keys, const uint8_t* item_in,
                              const uint64_t* rows, const double* score, const uint8_t* source, const uint32_t* count,
                              const double* planes_f64, uint32_t n_f64, const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32,
                              uint64_t* out_rows, double* out_score, uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask,
                              float* out_planes_f32, uint32_t* out_count) {
    const char* who = "pg_candidates_dimcap_host";
    const pg::CandCall l{rows, score, source, count, planes_f64, n_f64, source_mask, planes_f32, n_f32, out_rows, out_score,
                         out_source, out_planes_f64, out_source_mask, out_planes_f32, out_count};
    int rc;
    if ((rc = pg::cand_call_required(l, conf && keys, who)) || (rc = pg::dimcap_check_conf(conf, who)) || (rc = pg::cand_check_nq(nq, who)) ||
        (rc = pg::dimcap_check_cap(cap, who)) || (rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) ||
        (rc = pg::cand_call_apart(l, nq, cap, cap, who)))
        return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, cap, &in, &out);
    const bool null_as_value = conf->null_mode == PG_DIMCAP_NULL_VALUE;
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t q0 = (size_t)q * cap;
        const uint32_t n_valid = pg::cand_n_valid(in, q);
        std::unordered_map<int64_t, uint32_t> kept;                  // per value: the entries kept so far
        uint32_t kept_null = 0, n = 0;
        for (uint32_t p = 0; p < n_valid; ++p) {
            if (rows[q0 + p] == pg::kCandPad) continue;
            const bool null = (item_in && !item_in[q0 + p]) || (conf->has_null && keys[q0 + p] == conf->null_value);
            if (null && !null_as_value) {
                pg::cand_carry(in, out, q0 + p, q0 + n++, true);
                continue;
            }
            uint32_t& have = null ? kept_null : kept[keys[q0 + p]];
            if (have >= conf->limit) continue;
            ++have;
            pg::cand_carry(in, out, q0 + p, q0 + n++, true);
        }
        pg::cand_pad(in, out, q, n, 1, pg::kCandNan);
        out_count[q] = n;
    }
    return PG_OK;
}

int pg_candidates_dimcap_dev(pg_ctx* ctx, const pg_features* fs, const pg_dimcap_conf* conf, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                             const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                             uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                             double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                             float* d_out_planes_f32, uint32_t* d_out_count) {
    const char* who = "pg_candidates_dimcap_dev";
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    int rc;
    if ((rc = pg::cand_call_required(l, ctx && fs && conf && conf->column, who)) || (rc = pg::dimcap_check_conf(conf, who)) ||
        (rc = pg::cand_check_nq(nq, who)) || (rc = pg::dimcap_check_cap(cap, who)) || (rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) ||
        (rc = pg::cand_call_apart(l, nq, cap, cap, who)))
        return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::dimcap_locked(ctx, fs, conf, in, out, nullptr, who);
}

// ---- one request on host arrays (staged_run, cand_lists.hpp) ---------------------------------------------------------------------
int pg_candidates_dimcap(pg_ctx* ctx, const pg_features* fs, const pg_dimcap_conf* conf, uint32_t n, const uint64_t* rows, const double* score,
                         const uint8_t* source, uint64_t* out_rows, double* out_score, uint8_t* out_source, uint32_t* out_count) {
    const char* who = "pg_candidates_dimcap";
    PG_REQUIRE(ctx && fs && conf && conf->column && out_count && (n == 0 || (rows && score && out_rows && out_score)), "%s: NULL argument", who);
    int rc;
    if ((rc = pg::dimcap_check_conf(conf, who))) return rc;
    PG_REQUIRE(!source == !out_source, "%s: source and out_source come in pairs", who);
    if (n == 0) {                                    // an empty request: an empty answer
        *out_count = 0;
        return PG_OK;
    }
    if ((rc = pg::dimcap_check_cap(n, who))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kTable, kRows, kScore, kOutRows, kOutScore, kSource, kOutSource, kCount };
    Staged st[] = {{nullptr, 0, Staged::kSkip, pg::dimcap_table_bytes(1, n)},
                   {rows, (size_t)n * 8, Staged::kIn},       {score, (size_t)n * 8, Staged::kIn},   {out_rows, (size_t)n * 8, Staged::kOut},
                   {out_score, (size_t)n * 8, Staged::kOut}, {source, n, Staged::in_if(source)},    {out_source, n, Staged::out_if(source)},
                   {out_count, 4, Staged::kOut}};
    return pg::staged_run(ctx, pg::kSlotDimcap, st, sizeof st / sizeof *st, false, [&] {
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
        return pg::dimcap_locked(ctx, fs, conf, in, out, st[kTable].dev, who);
    });
}

}  // extern "C"
