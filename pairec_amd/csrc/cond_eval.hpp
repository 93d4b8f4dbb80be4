// cond_eval.hpp — what the per-candidate evaluators over feature-store columns share: cond.hip (FilterParam terms and boost
// expressions), classcut.hip (boolean class expressions, 4.1r) and mixsort.hip (a FilterParam rule per strategy,
// 4.1t).  A candidate is its row; the lane loads the raw bits of every referenced column before anything uses one and keeps
// them in registers; a column is read as float64(value).
//
// In this order: the candidate and its column reads; the by-name binding of a set's columns to a store; SetTable, the device
// table every compiled set (pg_cond, pg_classcut, pg_mix) owns; FilterParam compiled — the terms and rules, the pg_cond object
// and its bind to a store — which cond.hip and mixsort.hip walk.
#pragma once
#include "cand_lists.hpp"
#include "expr_prog.hpp"

#include <cstring>
#include <initializer_list>
#include <mutex>
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
        default: return cand_bits_f64(b);
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

// the device table of a compiled set: its lists and programs, uploaded at the first device call and owned until the set is freed
struct SetTable {
    struct Part { const void* host; size_t bytes; };
    std::mutex mu;                                // the upload: contexts on one device may share a set
    int device = -1;
    void* d = nullptr;
    size_t off[2] = {0, 0};                       // where each part begins (256-byte aligned)

    // the parts are on the context's device after this; caller holds ctx->mu.  The first call of a set allocates and uploads
    // (the only synchronous step; every later call only launches), a context on another device is refused.
    int ensure(pg_ctx* ctx, const char* who, std::initializer_list<Part> parts) {
        std::lock_guard<std::mutex> guard(mu);
        if (device >= 0 && device != ctx->device) {
            set_error("%s: the set's table lives on device %d, the context on device %d", who, device, ctx->device);
            return PG_ERR_INVALID;
        }
        if (device >= 0) return PG_OK;
        size_t end = 0, n = 0;
        for (const Part& p : parts) {
            off[n++] = end = align_up(end);
            end += p.bytes;
        }
        void* t = nullptr;
        PG_HIP(hipMalloc(&t, end + 256));
        hipError_t e = hipSuccess;
        n = 0;
        for (const Part& p : parts) {
            if (e == hipSuccess && p.bytes) e = hipMemcpy((char*)t + off[n], p.host, p.bytes, hipMemcpyHostToDevice);
            ++n;
        }
        if (e != hipSuccess) {
            hipFree(t);
            set_error("%s: uploading the set's table failed: %s", who, hipGetErrorString(e));
            return PG_ERR_DEVICE;
        }
        d = t;
        device = ctx->device;
        return PG_OK;
    }
    template <class T>
    const T* part(size_t i) const { return (const T*)((const char*)d + off[i]); }
    void release() {
        if (!d) return;
        int cur = 0;
        hipGetDevice(&cur);
        hipSetDevice(device);
        hipDeviceSynchronize();                     // (a launch that reads the table may still be in flight)
        hipFree(d);
        hipSetDevice(cur);
        d = nullptr;
    }
};


// ---- module.FilterParam compiled: what cond.hip (filter, boost) and mixsort.hip (strategy membership) walk -------------------------
constexpr uint32_t kCondMaxRules = 8, kCondMaxTerms = 8, kCondMaxSlots = 8, kCondMaxList = 64;      // (kCondMaxCols: above)
constexpr uint32_t kCondMaxExprOps = 64, kCondMaxExprDepth = 8;
static_assert(kCondMaxRules == PG_COND_MAX_RULES && kCondMaxTerms == PG_COND_MAX_TERMS &&
                  kCondMaxSlots == PG_COND_MAX_SLOTS && kCondMaxList == PG_COND_MAX_LIST && kCondMaxExprOps == PG_COND_MAX_EXPR_OPS &&
                  kCondMaxExprDepth == PG_COND_MAX_EXPR_DEPTH,
              "include/pairec_gpu.h repeats these");

struct CondTerm {                                 // 24 bytes
    uint8_t op, type, rhs, user_left;             // pg_cond_op, pg_cond_type, pg_cond_rhs; left side: 0 = column `left`, 1 = user slot `left`
    uint8_t left, rhs_idx, depth, is_and;         // rhs_idx: user slot or referenced column; depth 1: a child of the bool in front
    union { long long i; double f; } c;           // the constant
    uint16_t list_off, list_n;                    // in / not_in: values [list_off, list_off + list_n) of the table, ascending
    uint32_t pad;
};
struct CondRule { uint8_t term_off, n_terms; uint16_t prog_off, prog_n, pad; };
struct CondProgram {                              // what both kernels and the host statement walk
    CondCol cols[kCondMaxCols];                   // the referenced columns (host statement: base = the caller's candidate-aligned array)
    CondTerm terms[kCondMaxRules * kCondMaxTerms];
    CondRule rules[kCondMaxRules];
    const long long* lists;
    const Instr* progs;
    uint32_t n_used, n_rules;
    uint64_t store_rows;
};

// the request's user slots (the candidate itself: CondItem, above)
struct CondUser {
    const unsigned long long* vals;               // [kCondMaxSlots] bits: int64 or fp64 by the slot's type
    uint32_t present;
};

__host__ __device__ __forceinline__ long long cond_col_i64(const CondProgram& p, const CondItem& it, uint32_t k) {
    const unsigned long long b = cond_pick(it.raw, k);
    return p.cols[k].dtype == PG_F_I32 ? (long long)(int32_t)(uint32_t)b : (long long)b;          // (integer columns: the compiler checked)
}
// one operator that is not a bool (see the file header for where every answer comes from)
__host__ __device__ __forceinline__ bool cond_term(const CondProgram& p, const CondTerm& t, const CondItem& it, const CondUser& u) {
    const bool left_in = t.user_left ? ((u.present >> t.left) & 1u) != 0 : it.item_in;
    if (t.op == PG_COND_IS_NULL) return !left_in;
    if (t.op == PG_COND_IS_NOT_NULL) return left_in;
    if (!left_in) return t.op == PG_COND_NOT_EQUAL;
    const bool is_float = t.type == PG_COND_FLOAT;
    if (t.op == PG_COND_EQUAL || t.op == PG_COND_NOT_EQUAL) {
        if (is_float) return false;
    } else if (t.op == PG_COND_IN || t.op == PG_COND_NOT_IN) {
        if (is_float || t.type == PG_COND_INT64) return false;
        const long long v = t.user_left ? (long long)u.vals[t.left] : cond_col_i64(p, it, t.left);
        uint32_t lo = 0, hi = t.list_n;                               // the first value >= v
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (p.lists[t.list_off + mid] < v) lo = mid + 1; else hi = mid;
        }
        const bool found = lo < t.list_n && p.lists[t.list_off + lo] == v;
        return t.op == PG_COND_IN ? found : !found;
    }
    // the right-hand side
    if (t.rhs == PG_COND_RHS_USER && !((u.present >> t.rhs_idx) & 1u)) return t.op == PG_COND_NOT_EQUAL;
    if (t.rhs == PG_COND_RHS_ITEM && !it.item_in) return t.op == PG_COND_NOT_EQUAL || (t.op >= PG_COND_GREATER && is_float);
    if (is_float) {
        const double l = t.user_left ? cand_bits_f64(u.vals[t.left]) : cond_col_f64(p, it, t.left);
        const double r = t.rhs == PG_COND_RHS_USER ? cand_bits_f64(u.vals[t.rhs_idx])
                         : t.rhs == PG_COND_RHS_ITEM ? cond_col_f64(p, it, t.rhs_idx) : t.c.f;
        switch (t.op) {
            case PG_COND_GREATER: return l > r;
            case PG_COND_GREATER_THAN: return l >= r;
            case PG_COND_LESS: return l < r;
            default: return l <= r;
        }
    }
    const long long l = t.user_left ? (long long)u.vals[t.left] : cond_col_i64(p, it, t.left);
    const long long r = t.rhs == PG_COND_RHS_USER ? (long long)u.vals[t.rhs_idx] : t.rhs == PG_COND_RHS_ITEM ? cond_col_i64(p, it, t.rhs_idx) : t.c.i;
    switch (t.op) {
        case PG_COND_EQUAL: return l == r;
        case PG_COND_NOT_EQUAL: return l != r;
        case PG_COND_GREATER: return l > r;
        case PG_COND_GREATER_THAN: return l >= r;
        case PG_COND_LESS: return l < r;
        default: return l <= r;
    }
}

// FilterParam.EvaluateByDomain of rule r (filter_op.go:507-540; a bool's children: :1679-1756)
__host__ __device__ __forceinline__ bool cond_rule(const CondProgram& p, uint32_t r, const CondItem& it, const CondUser& u) {
    const uint32_t t0 = p.rules[r].term_off, t1 = t0 + p.rules[r].n_terms;
    bool all = true;
    uint32_t i = t0;
    while (i < t1) {
        const CondTerm& t = p.terms[i];
        bool v;
        if (t.op == PG_COND_BOOL) {
            bool any = false, every = true;
            for (++i; i < t1 && p.terms[i].depth == 1; ++i) {
                const bool c = cond_term(p, p.terms[i], it, u);
                any = any || c;
                every = every && c;
            }
            v = t.is_and ? every : any;
        } else {
            v = cond_term(p, t, it, u);
            ++i;
        }
        all = all && v;
    }
    return all;
}

}  // namespace pg

// the compiled object (pg_cond_compile, cond.hip)
struct pg_cond {
    bool boost = false;
    std::vector<std::string> col_names;           // as declared
    std::vector<int> col_dtypes;
    std::vector<int> used;                        // referenced columns → declared index (<= kCondMaxCols)
    std::vector<std::string> slot_names;          // user slots in order of first use
    std::vector<uint8_t> slot_float;
    std::vector<pg::CondTerm> terms;
    std::vector<pg::CondRule> rules;
    std::vector<long long> lists;
    std::vector<pg::Instr> progs;
    pg::SetTable table;                           // lists | programs
};

namespace pg {

// the kernel argument / the host statement's program; cols_base[k]: the base of referenced column k
inline void cond_program(const pg_cond* c, const void* const* declared_base, const long long* lists, const Instr* progs, uint64_t store_rows, CondProgram* p) {
    memset(p, 0, sizeof *p);
    for (size_t k = 0; k < c->used.size(); ++k) p->cols[k] = CondCol{declared_base[c->used[k]], c->col_dtypes[(size_t)c->used[k]], 0};
    std::copy(c->terms.begin(), c->terms.end(), p->terms);
    std::copy(c->rules.begin(), c->rules.end(), p->rules);
    p->lists = lists;
    p->progs = progs;
    p->n_used = (uint32_t)c->used.size();
    p->n_rules = (uint32_t)c->rules.size();
    p->store_rows = store_rows;
}

inline int cond_host_check(const pg_cond* c, const void* const* cols, const uint64_t* user_vals, const char* who) {
    for (int d : c->used)
        if (!cols || !cols[d]) {
            set_error("%s: the values of column \"%s\" are missing", who, c->col_names[(size_t)d].c_str());
            return PG_ERR_INVALID;
        }
    if (!c->slot_names.empty() && !user_vals) {
        set_error("%s: the set reads user property \"%s\" but user_vals is NULL", who, c->slot_names[0].c_str());
        return PG_ERR_INVALID;
    }
    return PG_OK;
}

// binds the set to a store by name and makes sure its table is on the context's device; caller holds ctx->mu
inline int cond_bind_locked(pg_ctx* ctx, pg_cond* c, const pg_features* fs, const char* who, CondProgram* p) {
    std::vector<const void*> declared;
    int rc;
    if ((rc = cond_resolve_columns(fs, c->col_names, c->col_dtypes, c->used, who, &declared))) return rc;
    if ((rc = c->table.ensure(ctx, who, {{c->lists.data(), c->lists.size() * 8}, {c->progs.data(), c->progs.size() * sizeof(Instr)}}))) return rc;
    cond_program(c, declared.data(), c->table.part<long long>(0), c->table.part<Instr>(1), fs->rows, p);
    return PG_OK;
}

}  // namespace pg
