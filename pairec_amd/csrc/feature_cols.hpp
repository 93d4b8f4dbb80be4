// feature_cols.hpp — how a kernel reads a typed feature column (features.hip owns the columns; rank_gbdt.hip reads them too).
#pragma once
#include "common.hpp"

namespace pg {

struct ColDesc {
    const void* base;
    int32_t dtype;
    int32_t pad;
    double def;
};

// (float)value with ONE rounding: an integer converts to fp32 directly — through a double an int64 beyond 2^53 rounds twice
// (2^60 + 2^36 + 1 is 0x5D800001 directly, 0x5D800000 by way of the double).  The stored default (pg_features_set_column) is
// already a value of the column's dtype, exact in the double that carries it.
__device__ __forceinline__ float load_as_f32(const ColDesc& c, uint32_t row, uint64_t rows) {
    if (row >= rows) return (float)c.def;
    switch (c.dtype) {
        case PG_F_I32: return (float)((const int32_t*)c.base)[row];
        case PG_F_I64: return (float)((const int64_t*)c.base)[row];
        case PG_F_F32: return ((const float*)c.base)[row];
        default: return (float)((const double*)c.base)[row];
    }
}

}  // namespace pg
