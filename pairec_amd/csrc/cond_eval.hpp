// cond_eval.hpp — what the per-candidate evaluators over feature-store columns share: cond.hip (FilterParam terms and boost
// expressions) and classcut.hip (boolean class expressions, 4.1r).  A candidate is its row; the lane loads the
// raw bits of every referenced column before anything uses one and keeps them in registers; a column is read as float64(value).
#pragma once
#include "cand_lists.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace pg {

constexpr uint32_t kCondMaxCols = 16;
static_assert(kCondMaxCols == PG_COND_MAX_COLS, "include/pairec_gpu.h repeats this");

struct CondCol { const void* base; int32_t dtype; int32_t pad; };

// the candidate as the evaluators see it: raw bits of every referenced column (meaningful iff item_in)
struct CondItem {
    unsigned long long raw[kCondMaxCols];
    bool item_in;
};

// r[k] for a wave-uniform k as a chain of selects over constant indices: the values stay in registers.  (Left to itself the
// optimiser folds the chain back into one indexed read, which puts the array in scratch; the empty asm keeps the links apart.)
template <int N>
__host__ __device__ __forceinline__ unsigned long long cond_pick(const unsigned long long (&r)[N], uint32_t k) {
    unsigned long long v = r[0];
#pragma unroll
    for (int j = 1; j < N; ++j) {
        v = k == (uint32_t)j ? r[j] : v;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));
#endif
    }
    return v;
}
__host__ __device__ __forceinline__ double cond_bits_f64(unsigned long long b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
// referenced column k as float64(value); P: a program with cols[kCondMaxCols]
template <class P>
__host__ __device__ __forceinline__ double cond_col_f64(const P& p, const CondItem& it, uint32_t k) {
    const unsigned long long b = cond_pick(it.raw, k);
    switch (p.cols[k].dtype) {
        case PG_F_I32: return (double)(int32_t)(uint32_t)b;
        case PG_F_I64: return (double)(long long)b;
        case PG_F_F32: {
            const uint32_t w = (uint32_t)b;
            float f;
            memcpy(&f, &w, 4);
            return (double)f;
        }
        default: return cond_bits_f64(b);
    }
}

// the referenced columns of `row`, every load issued before anything uses one; P: cols, n_used, store_rows
template <class P>
__device__ __forceinline__ void cond_load(const P& p, unsigned long long row, CondItem* it) {
    it->item_in = row < p.store_rows;
#pragma unroll
    for (uint32_t k = 0; k < kCondMaxCols; ++k) {
        unsigned long long b = 0;
        if (k < p.n_used && it->item_in) {
            const int dt = p.cols[k].dtype;
            if (dt == PG_F_I32 || dt == PG_F_F32) b = ((const uint32_t*)p.cols[k].base)[row];
            else b = ((const unsigned long long*)p.cols[k].base)[row];
        }
        it->raw[k] = b;
    }
}

// host statements: the candidate's values from candidate-aligned arrays; used[k]: the declared column behind referenced column k
inline void cond_host_item(const std::vector<int>& used, const std::vector<int>& col_dtypes, const void* const* cols, const uint8_t* item_in,
                           size_t i, CondItem* it) {
    it->item_in = item_in ? item_in[i] != 0 : true;
    for (uint32_t k = 0; k < kCondMaxCols; ++k) {
        unsigned long long b = 0;
        if (k < used.size() && it->item_in) {
            const int d = used[k], dt = col_dtypes[(size_t)d];
            if (dt == PG_F_I32 || dt == PG_F_F32) b = ((const uint32_t*)cols[d])[i];
            else b = ((const unsigned long long*)cols[d])[i];
        }
        it->raw[k] = b;
    }
}

// the referenced declared columns bound by name to a store: declared[d] = the store's values of declared column d
inline int cond_resolve_columns(const pg_features* fs, const std::vector<std::string>& col_names, const std::vector<int>& col_dtypes,
                                const std::vector<int>& used, const char* who, std::vector<const void*>* declared) {
    declared->assign(col_names.size(), nullptr);
    for (int d : used) {
        const pg_features::Column* col = nullptr;
        for (const auto& x : fs->cols)
            if (x.name == col_names[(size_t)d]) { col = &x; break; }
        if (!col || !col->d) {
            set_error("%s: column \"%s\" is not a column of the feature store", who, col_names[(size_t)d].c_str());
            return PG_ERR_INVALID;
        }
        if (col->dtype != col_dtypes[(size_t)d]) {
            set_error("%s: column \"%s\" has dtype %d in the feature store, the set was compiled for dtype %d", who, col->name.c_str(), col->dtype,
                      col_dtypes[(size_t)d]);
            return PG_ERR_INVALID;
        }
        (*declared)[(size_t)d] = col->d;
    }
    return PG_OK;
}

inline int cond_check_shape(uint32_t nq, uint32_t cap, const char* who) {
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    if (cap < 1 || cap > kCandMaxCap) {
        set_error("%s: cap=%u unsupported (1..%u)", who, cap, kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}

// [a, a + an) and [b, b + bn) share a byte
inline bool cond_overlap(const void* a, size_t an, const void* b, size_t bn) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

}  // namespace pg
