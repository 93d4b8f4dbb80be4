// recall_filter.hip — a recall over the rows a filter admits: a Hologres vector recall WITH its WhereClause
// (HologresVectorConf.WhereClause, recconf.go:492-497; hologres_vector_recall.go:23,56-61 / hologres_vector_recall_v2.go:23).
// Counting the admitted rows, their stable compaction into a compact table or a view of the table, the map from a compact
// table's rows back to the source's, and the searches built on them (recall_where_locked, pg_recall_topk_where,
// pg_table_view_create).  The filter inside the table pass itself is recall.hip's; compound clauses are where.hip's.
#include "common.hpp"
#include "recall_shared.hpp"
#include "block_rank.hpp"

namespace pg {

// rows that pass a recall's filter (one pass over the column: 0.4 GB per 100 M rows)
__global__ void filter_count_kernel(RowFilter f, uint64_t rows, unsigned long long* __restrict__ out) {
    unsigned long long n = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x)
        n += row_filter_pass(f, (uint32_t)r) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

// ---- selective filters: the admitted rows, in row order (stable compaction), gathered into a compact table ----
constexpr uint32_t kCompactBlockRows = 1024;
__device__ __forceinline__ bool filter_cmp(int op, long long v, long long val) {
    switch (op) {
        case 0: return v > val;
        case 1: return v >= val;
        case 2: return v < val;
        case 3: return v <= val;
        case 4: return v == val;
        default: return v != val;
    }
}
// bit i: row r0 + i passes (r0 a multiple of 4: one 16-B load of an int32 column, two of an int64 one, four bits of a bitmap)
__device__ __forceinline__ uint32_t row_filter_mask4(const RowFilter& f, uint64_t r0, uint64_t rows) {
    uint32_t m = 0;
    if (f.dtype == kFilterBits) return (reinterpret_cast<const uint32_t*>(f.col)[r0 >> 5] >> (uint32_t)(r0 & 31u)) & 0xFu;   // (zero bits beyond the rows)
    if (r0 + 4 <= rows) {
        if (f.dtype == PG_F_I64) {
            const longlong2 a = reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(f.col) + r0)[0];
            const longlong2 b = reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(f.col) + r0)[1];
            m = (filter_cmp(f.op, a.x, f.val) ? 1u : 0u) | (filter_cmp(f.op, a.y, f.val) ? 2u : 0u) | (filter_cmp(f.op, b.x, f.val) ? 4u : 0u) |
                (filter_cmp(f.op, b.y, f.val) ? 8u : 0u);
        } else {
            const int4 a = *reinterpret_cast<const int4*>(reinterpret_cast<const int32_t*>(f.col) + r0);
            m = (filter_cmp(f.op, a.x, f.val) ? 1u : 0u) | (filter_cmp(f.op, a.y, f.val) ? 2u : 0u) | (filter_cmp(f.op, a.z, f.val) ? 4u : 0u) |
                (filter_cmp(f.op, a.w, f.val) ? 8u : 0u);
        }
    } else {
        for (uint32_t i = 0; i < 4 && r0 + i < rows; ++i) m |= row_filter_pass(f, (uint32_t)(r0 + i)) ? 1u << i : 0u;
    }
    return m;
}
__global__ __launch_bounds__(256) void filter_block_count_kernel(RowFilter f, uint64_t rows, uint32_t* __restrict__ block_n) {
    __shared__ uint32_t ws[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * kCompactBlockRows + threadIdx.x * 4;
    uint32_t n = r0 < rows ? (uint32_t)__popc(row_filter_mask4(f, r0, rows)) : 0u;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) block_n[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
// The block counts' exclusive scan in two parallel levels: every group of 1024 counts is scanned in place by a workgroup of its
// own (its total → group_n[g]); one small workgroup then scans the <= 4096 group totals (grand total → group_n[ngroups]).  A
// block's offset is block_n[b] + group_n[b / 1024].
__global__ __launch_bounds__(1024) void filter_group_scan_kernel(uint32_t* __restrict__ block_n, uint32_t n, uint32_t* __restrict__ group_n) {
    __shared__ uint32_t wsum[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    const uint32_t v = i < n ? block_n[i] : 0u;
    uint32_t total;
    const uint32_t excl = block_excl_scan<16>(v, wsum, &total);
    if (i < n) block_n[i] = excl;
    if (threadIdx.x == 0) group_n[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void filter_total_scan_kernel(uint32_t* __restrict__ group_n, uint32_t ngroups) {
    __shared__ uint32_t wsum[16];
    uint32_t v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x * 4 + j;
        v[j] = i < ngroups ? group_n[i] : 0u;
        s += v[j];
    }
    uint32_t total;
    uint32_t acc = block_excl_scan<16>(s, wsum, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x * 4 + j;
        if (i < ngroups) group_n[i] = acc;
        acc += v[j];
    }
    if (threadIdx.x == 0) group_n[ngroups] = total;
}
// ids[block offset + rank inside the block] = row, ranks in row order: a thread takes 4 consecutive rows, a wave 256
__global__ __launch_bounds__(256) void filter_scatter_kernel(RowFilter f, uint64_t rows, const uint32_t* __restrict__ block_off,
                                                             const uint32_t* __restrict__ group_off, uint32_t* __restrict__ ids) {
    __shared__ uint32_t wn[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * kCompactBlockRows + threadIdx.x * 4;
    const uint32_t m = r0 < rows ? row_filter_mask4(f, r0, rows) : 0u;
    uint32_t total;
    uint32_t pos = block_off[blockIdx.x] + group_off[blockIdx.x >> 10] + block_excl_scan<4>((uint32_t)__popc(m), wn, &total);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (m & (1u << i)) ids[pos++] = (uint32_t)(r0 + i);
}
// compact[i][:] = tab[ids[i]][:] (a wave per row-quad: 16 B per lane)
__global__ void compact_gather_kernel(const float* __restrict__ tab, const uint32_t* __restrict__ ids, uint32_t n, uint32_t dim,
                                      float* __restrict__ out) {
    const uint32_t q4 = dim / 4;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n * q4) return;
    const uint32_t r = (uint32_t)(i / q4), c = (uint32_t)(i % q4);
    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(tab + (size_t)ids[r] * dim)[c];
}
__global__ void compact_gather_nx_kernel(const float* __restrict__ nx, const uint32_t* __restrict__ ids, uint32_t n, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n + 64) out[i] = i < n ? nx[ids[i]] : 0.0f;
}
__global__ void recall_pad_kernel(uint64_t* __restrict__ rows, float* __restrict__ scores, size_t n, bool l2) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        rows[i] = ~0ull;
        scores[i] = l2 ? __builtin_inff() : -__builtin_inff();
    }
}
// local rows of the compact table → the table's global row ids (padding stays UINT64_MAX)
__global__ void compact_map_rows_kernel(uint64_t* __restrict__ rows, uint64_t n, const uint32_t* __restrict__ ids, uint64_t row_offset,
                                        uint64_t n_ids) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && rows[i] < n_ids) rows[i] = row_offset + ids[rows[i]];      // (padding, UINT64_MAX, stays)
}

// the two kernels of this file that the plans of recall_plan.hip launch (declared in recall_shared.hpp)
int filter_count_launch(pg_ctx* ctx, const RowFilter& filter, uint64_t rows, unsigned long long* d_n) {
    filter_count_kernel<<<(uint32_t)ctx->num_cus * 8, 256, 0, ctx->stream>>>(filter, rows, d_n);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
int compact_map_rows_launch(pg_ctx* ctx, uint64_t* d_rows, uint64_t n, const uint32_t* ids, uint64_t offset, uint64_t rows) {
    compact_map_rows_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, ctx->stream>>>(d_rows, n, ids, offset, rows);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// Count the rows `f` admits per 1024-row block (one pass over the column) and scan the counts — the scan is also the compaction's
// map (filter_scatter_kernel); buffers in kSlotFilterCount.  Synchronises the stream (the count comes back to the host).
int filter_count_locked(pg_ctx* ctx, const RowFilter& f, uint64_t rows, uint32_t** d_blk_out, uint32_t** d_grp_out, uint32_t* cblocks_out,
                        uint32_t* admitted_out) {
    const uint32_t cblocks = (uint32_t)((rows + kCompactBlockRows - 1) / kCompactBlockRows);
    const uint32_t cgroups = (cblocks + 1023) / 1024;
    if (cgroups > 4096) {
        set_error("filtered recall: table of %llu rows too large", (unsigned long long)rows);
        return PG_ERR_UNSUPPORTED;
    }
    uint32_t *d_blk, *d_grp; int rc;
    if ((rc = scratch_carve(ctx, kSlotFilterCount, [&](Carve& c) {
            d_blk = c.take<uint32_t>(cblocks);
            d_grp = c.take<uint32_t>((size_t)cgroups + 2);      // the groups' scan, the total behind it
        }))) return rc;
    uint32_t admitted = 0;
    if (cblocks) {
        filter_block_count_kernel<<<cblocks, 256, 0, ctx->stream>>>(f, rows, d_blk);
        filter_group_scan_kernel<<<cgroups, 1024, 0, ctx->stream>>>(d_blk, cblocks, d_grp);
        filter_total_scan_kernel<<<1, 1024, 0, ctx->stream>>>(d_grp, cgroups);
        PG_HIP(hipGetLastError());
        PG_HIP(hipMemcpyAsync(&admitted, d_grp + cgroups, 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
    }
    *d_blk_out = d_blk;
    *d_grp_out = d_grp;
    *cblocks_out = cblocks;
    *admitted_out = admitted;
    return PG_OK;
}

int where_check(const char* who, const pg_ctx* ctx, const pg_table* t, const pg_features* fs, int column, int op, long long value,
                int metric, const void* queries, const void* rows, const void* scores, uint32_t nq, uint32_t k, RowFilter* f) {
    PG_REQUIRE(ctx && t && fs && queries && rows && scores, "%s: NULL argument", who);
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    PG_REQUIRE(t->dim <= 128 || nq <= 32, "%s: dim %u supports at most 32 queries per call", who, t->dim);
    PG_REQUIRE(column >= 0 && (size_t)column < fs->cols.size(), "%s: column %d out of range", who, column);
    PG_REQUIRE(op >= 0 && op <= 5, "%s: op %d unknown (0 >, 1 >=, 2 <, 3 <=, 4 ==, 5 !=)", who, op);
    PG_REQUIRE(metric == 0 || metric == 1, "%s: metric %d unknown (0 inner product, 1 squared Euclidean)", who, metric);
    PG_REQUIRE(fs->rows >= t->rows, "%s: the feature store holds %llu rows, the table %llu", who, (unsigned long long)fs->rows,
               (unsigned long long)t->rows);
    const pg_features::Column& c = fs->cols[(size_t)column];
    if ((c.dtype != PG_F_I32 && c.dtype != PG_F_I64) || !c.d) {
        set_error("%s: column \"%s\" must be an int32 / int64 column with values", who, c.name.c_str());
        return PG_ERR_UNSUPPORTED;
    }
    if (k < 1 || k > 16384) {
        set_error("%s: k=%u unsupported (1..16384)", who, k);
        return PG_ERR_UNSUPPORTED;
    }
    *f = RowFilter();
    f->col = c.d;
    f->dtype = c.dtype;
    f->op = op;
    f->val = value;
    return PG_OK;
}

int where_pad_launch(pg_ctx* ctx, uint64_t* d_rows, float* d_sc, size_t n, bool l2) {
    recall_pad_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, ctx->stream>>>(d_rows, d_sc, n, l2);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int recall_where_locked(pg_ctx* ctx, const pg_table* t, RowFilter f, int metric, const float* d_q, uint32_t nq, uint32_t k,
                        uint64_t* d_rows, float* d_sc, uint32_t* out_count) {
    int rc;
    uint32_t *d_blk, *d_grp, cblocks, admitted;
    if ((rc = filter_count_locked(ctx, f, t->rows, &d_blk, &d_grp, &cblocks, &admitted))) return rc;
    f.admitted = admitted;
    if (admitted == 0) {
        // nothing passes: every slot is padding (row UINT64_MAX, score -inf / distance +inf), every count 0
        if ((rc = where_pad_launch(ctx, d_rows, d_sc, (size_t)nq * k, metric == 1))) return rc;
        if (out_count) for (uint32_t q = 0; q < nq; ++q) out_count[q] = 0;
    } else if (admitted <= (nq <= 4 ? ctx->knobs.where_compact_max_rows / 2 : ctx->knobs.where_compact_max_rows) &&
               (uint64_t)admitted * ctx->knobs.where_compact_min_ratio <= t->rows &&
               (metric == 0 || t->dim == 64 || t->dim == 128)) {
        // A selective filter: the thresholds the scan plans estimate from samples of the table say little about the few rows
        // that pass (1 % admitted of 100 M rows, 128 queries: 180 ms of re-planned passes).  Gather the admitted rows, in row
        // order, into a compact table and run the exact scan over that: its rows are the candidates, its row order the tie
        // order, and the answer's local rows map back through the id list.  (The gather is 1 KB of traffic per admitted row: at
        // 100 M x 128 the copy wins below ~4 M rows for a lone query — in place 2.2 ms at 4 % — and below ~8 M for 16+ queries.)
        uint32_t* d_ids;
        float *d_tab, *d_cnx = nullptr;
        if ((rc = scratch_carve(ctx, kSlotFilterGather, [&](Carve& c) {
                d_ids = c.take<uint32_t>((size_t)admitted + 64);
                d_tab = c.take<float>(((size_t)admitted + 64) * t->dim);
                if (metric == 1) d_cnx = c.take<float>((size_t)admitted + 64);
            }))) return rc;
        filter_scatter_kernel<<<cblocks, 256, 0, ctx->stream>>>(f, t->rows, d_blk, d_grp, d_ids);
        const uint64_t quads = (uint64_t)admitted * (t->dim / 4);
        compact_gather_kernel<<<(uint32_t)((quads + 255) / 256), 256, 0, ctx->stream>>>(t->d, d_ids, admitted, t->dim, d_tab);
        PG_HIP(hipMemsetAsync(d_tab + (size_t)admitted * t->dim, 0, (size_t)64 * t->dim * 4, ctx->stream));
        pg_table ct;
        ct.d = d_tab;
        ct.rows = admitted;
        ct.dim = t->dim;
        if (metric == 1) {
            if ((rc = ensure_table_nx(ctx, t))) return rc;
            compact_gather_nx_kernel<<<(admitted + 64 + 255) / 256, 256, 0, ctx->stream>>>(t->derived.d_nx, d_ids, admitted, d_cnx);
            ct.derived.d_nx = d_cnx;
            ct.derived.nx_valid = true;
        }
        PG_HIP(hipGetLastError());
        RecallOpts o;
        o.l2 = metric == 1;
        o.exact_only = true;
        if ((rc = recall_batches_locked(ctx, &ct, d_q, nq, k, d_rows, d_sc, out_count, o))) return rc;
        if ((rc = compact_map_rows_launch(ctx, d_rows, (uint64_t)nq * k, d_ids, t->row_offset, admitted))) return rc;
        ct.d = nullptr;
        ct.derived.d_nx = nullptr;
    } else {
        RecallOpts o;
        o.l2 = metric == 1;
        o.filter = &f;
        if ((rc = recall_batches_locked(ctx, t, d_q, nq, k, d_rows, d_sc, out_count, o))) return rc;
    }
    return PG_OK;
}

int view_create_locked(const char* who, pg_ctx* ctx, const pg_table* t, const RowFilter& f, pg_table** out_view) {
    PG_HIP(hipSetDevice(ctx->device));
    int rc;
    uint32_t *d_blk, *d_grp, cblocks, admitted;
    if ((rc = filter_count_locked(ctx, f, t->rows, &d_blk, &d_grp, &cblocks, &admitted))) return rc;
    if (admitted == 0) {
        set_error("%s: no row passes the filter", who);
        return PG_ERR_EMPTY;
    }
    pg_table* v = new pg_table();
    v->rows = admitted;
    v->dim = t->dim;
    v->row_offset = 0;
    v->map_offset = t->row_offset;
    hipError_t e = hipMalloc((void**)&v->d, ((size_t)admitted + 64) * t->dim * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&v->d_row_map, ((size_t)admitted + 64) * sizeof(uint32_t));
    if (e != hipSuccess) {
        set_error("%s: hipMalloc(%.1f GB) failed: %s", who, (double)admitted * t->dim * 4 / 1e9, hipGetErrorString(e));
        if (v->d) (void)hipFree(v->d);
        delete v;
        return PG_ERR_NOMEM;
    }
    filter_scatter_kernel<<<cblocks, 256, 0, ctx->stream>>>(f, t->rows, d_blk, d_grp, v->d_row_map);
    const uint64_t quads = (uint64_t)admitted * (t->dim / 4);
    compact_gather_kernel<<<(uint32_t)((quads + 255) / 256), 256, 0, ctx->stream>>>(t->d, v->d_row_map, admitted, t->dim, v->d);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemsetAsync(v->d + (size_t)admitted * t->dim, 0, (size_t)64 * t->dim * sizeof(float), ctx->stream));
    PG_HIP(hipMemsetAsync(v->d_row_map + admitted, 0, 64 * sizeof(uint32_t), ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    *out_view = v;
    return PG_OK;
}

}  // namespace pg

extern "C" {

// A Hologres vector recall WITH its WhereClause (HologresVectorConf.WhereClause, recconf.go:492-497; the SQL of
// hologres_vector_recall.go:23 / hologres_vector_recall_v2.go:23 has `FROM table WHERE … ORDER BY distance`), in the shape the
// device serves: `column OP constant` over an integer feature column keyed by item row (e.g. "create_time > ${time}" with the
// constant substituted by the caller, as :56-61 does).  metric 0: inner product, descending; 1: squared Euclidean, ascending.
// Only rows that pass are candidates; out_count[q] = min(k, rows that pass).  Exact, like the unfiltered recalls: the predicate
// is applied where candidates are made, so the plans' thresholds are thresholds of the filtered top-K.
int pg_recall_topk_where(pg_ctx* ctx, const pg_table* t, const pg_features* fs, int column, int op, long long value, int metric,
                         const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    pg::RowFilter f;
    int rc;
    if ((rc = pg::where_check("pg_recall_topk_where", ctx, t, fs, column, op, value, metric, queries, out_rows, out_scores, nq, k, &f)))
        return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    pg_index* ix = pg::index_route_where(ctx, t);          // ("index_route_where": the attached index, when it is current)
    uint32_t counts[pg::kMaxQueries];
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return ix ? pg::index_where_locked(ctx, ix, pg::WhereId{fs, column, nullptr, 0}, f, metric == 1, d_q, nq, k, d_rows, d_sc, counts)
                  : pg::recall_where_locked(ctx, t, f, metric, d_q, nq, k, d_rows, d_sc, counts);
    };
    if ((rc = pg::recall_staged(ctx, t->dim, queries, nq, k, out_rows, out_scores, run))) return rc;
    if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
    return PG_OK;
}

// A filtered VIEW of a table: the rows `column OP value` admits, in row order, copied into a table of their own whose recalls
// answer with the source's row ids.  What a Hologres recall with a WhereClause whose constant is fixed when the recall is built
// (hologres_vector_recall.go:56-61: "${time}" is substituted in the constructor) searches: build the view once per table
// generation and every recall flavour — pg_recall_topk[_l2][_dev], a coalescer's pg_coalescer_recall[_l2] — serves it at the speed
// of an unfiltered table of that size (own shadows, statistics and threshold model).  A snapshot: later changes of the source or
// the column do not reach it.  Ties break by source row, as in pg_recall_topk_where.  Destroyed with pg_table_destroy.
int pg_table_view_create(pg_ctx* ctx, const pg_table* t, const pg_features* fs, int column, int op, long long value, pg_table** out_view) {
    PG_REQUIRE(ctx && t && fs && out_view, "pg_table_view_create: NULL argument");
    PG_REQUIRE(!t->d_row_map, "pg_table_view_create: the source is a view itself");
    PG_REQUIRE(column >= 0 && (size_t)column < fs->cols.size(), "pg_table_view_create: column %d out of range", column);
    PG_REQUIRE(op >= 0 && op <= 5, "pg_table_view_create: op %d unknown (0 >, 1 >=, 2 <, 3 <=, 4 ==, 5 !=)", op);
    PG_REQUIRE(fs->rows >= t->rows, "pg_table_view_create: the feature store holds %llu rows, the table %llu", (unsigned long long)fs->rows,
               (unsigned long long)t->rows);
    const pg_features::Column& c = fs->cols[(size_t)column];
    if ((c.dtype != PG_F_I32 && c.dtype != PG_F_I64) || !c.d) {
        pg::set_error("pg_table_view_create: column \"%s\" must be an int32 / int64 column with values", c.name.c_str());
        return PG_ERR_UNSUPPORTED;
    }
    pg::RowFilter f;
    f.col = c.d;
    f.dtype = c.dtype;
    f.op = op;
    f.val = value;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    return pg::view_create_locked("pg_table_view_create", ctx, t, f, out_view);
}

}  // extern "C"
