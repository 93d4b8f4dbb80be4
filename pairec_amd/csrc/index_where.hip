// index_where.hip — the lists of an exact IVF index restricted to the rows a filter admits: built on the
// device, kept per index in a small LRU cache whose policy is index_serve.hpp's.  The search over them is index.hip's.
#include "index_shared.hpp"
#include "block_rank.hpp"

#include <hipcub/hipcub.hpp>

namespace pg {
namespace {

// bit r of bits: row r passes the filter.  Rows in order (the column is read coalesced); a wave's 64 rows are two words.
__global__ __launch_bounds__(256) void where_bits_kernel(RowFilter f, uint64_t rows, uint32_t* __restrict__ bits) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool pass = r < rows && row_filter_pass(f, (uint32_t)r);
    const uint64_t m = __builtin_amdgcn_ballot_w64(pass);
    if ((threadIdx.x & 63) == 0 && r < rows) {
        bits[r >> 5] = (uint32_t)m;
        if (r + 32 < rows) bits[(r >> 5) + 1] = (uint32_t)(m >> 32);
    }
}

// one block per list: the positions of list L whose row passes (bits[perm[p]], a gather from a bitmap of rows / 8 bytes).
// COUNT: cnt[L] = how many.  Else the stable compaction: perm_f[off_f[L] + rank] = perm[p], ranks in position order.
template <bool COUNT>
__global__ __launch_bounds__(256) void where_lists_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt_off,
                                                          uint32_t* __restrict__ perm_f) {
    __shared__ uint32_t wsum[4];
    const uint32_t L = blockIdx.x;
    const uint32_t b = off[L], e = off[L + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t base = COUNT ? 0u : cnt_off[L];
    for (uint32_t p0 = b; p0 < e; p0 += 256) {
        const uint32_t p = p0 + threadIdx.x;
        const uint32_t row = p < e ? perm[p] : 0u;
        const bool pass = p < e && ((bits[row >> 5] >> (row & 31)) & 1u);
        // (block_rank.hpp's wave_rank only: one set of counts and a barrier behind the reads — chunk_rank's two sets would
        // double this kernel's LDS words)
        uint32_t n_w;
        const uint32_t before = wave_rank(pass, &n_w);
        if (lane == 0) wsum[w] = n_w;
        __syncthreads();
        if (!COUNT && pass) {
            uint32_t pos = base + before;
            for (int j = 0; j < w; ++j) pos += wsum[j];
            perm_f[pos] = row;
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (COUNT && threadIdx.x == 0) cnt_off[L] = base;
}

// A filter's lists over the index, built on ctx->stream: the predicate's bitmap in row order, the admitted rows per list, their
// exclusive scan (the offsets), then the stable compaction of the permutation.  Synchronises (the total sizes the allocation).
int where_lists_build(pg_ctx* ctx, const pg_index* ix, const RowFilter& f, std::shared_ptr<WhereLists>* out) {
    const uint32_t nl = ix->n_lists;
    const uint64_t rows = ix->rows;
    hipStream_t s = ctx->stream;
    std::vector<void*> temp;
    auto done = [&](int rc) {
        (void)hipStreamSynchronize(s);
        free_all(temp);
        return rc;
    };
    int rc;
    uint32_t *bits = nullptr, *cnt, *off;
    const size_t words = (size_t)((rows + 31) / 32);
    const bool have_bits = f.dtype == kFilterBits;       // (a compound clause's filter IS the bitmap in row order)
    if ((!have_bits && (rc = dalloc((void**)&bits, words * 4, temp))) || (rc = dalloc((void**)&cnt, ((size_t)nl + 1) * 4, temp)) ||
        (rc = dalloc((void**)&off, ((size_t)nl + 1) * 4, temp)))
        return done(rc);
    size_t scan_b = 0;
    void* scan_tmp;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, cnt, off, nl + 1, s) != hipSuccess) return done(PG_ERR_DEVICE);
    if ((rc = dalloc(&scan_tmp, scan_b, temp))) return done(rc);
    if (have_bits) bits = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(f.col));
    else where_bits_kernel<<<(uint32_t)((rows + 255) / 256), 256, 0, s>>>(f, rows, bits);
    if (hipMemsetAsync(cnt + nl, 0, 4, s) != hipSuccess) return done(PG_ERR_DEVICE);
    where_lists_kernel<true><<<nl, 256, 0, s>>>(ix->a.perm, ix->a.off, bits, cnt, nullptr);
    if (hipGetLastError() != hipSuccess || hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_b, cnt, off, nl + 1, s) != hipSuccess)
        return done(PG_ERR_DEVICE);
    uint32_t admitted = 0;
    if (hipMemcpyAsync(&admitted, off + nl, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(PG_ERR_DEVICE);
    auto wl = std::make_shared<WhereLists>();
    const size_t off_b = align_up(((size_t)nl + 1) * 4);
    if (hipMalloc(&wl->d, off_b + (size_t)admitted * 4 + 16) != hipSuccess) {
        (void)hipGetLastError();
        wl->d = nullptr;
        return done(PG_ERR_NOMEM);
    }
    wl->off = (uint32_t*)wl->d;
    wl->perm = (uint32_t*)((char*)wl->d + off_b);
    wl->admitted = admitted;
    wl->bytes = (size_t)admitted * 4 + ((size_t)nl + 1) * 4;
    if (hipMemcpyAsync(wl->off, off, ((size_t)nl + 1) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return done(PG_ERR_DEVICE);
    where_lists_kernel<false><<<nl, 256, 0, s>>>(ix->a.perm, ix->a.off, bits, wl->off, wl->perm);
    if (hipGetLastError() != hipSuccess) return done(PG_ERR_DEVICE);
    rc = done(PG_OK);
    if (rc == PG_OK) *out = std::move(wl);
    return rc;
}

}  // namespace

// the filter's lists from the index's cache, or built (and kept while "index_where_cache" of the calling context allows); caller
// holds ctx->mu and the table's shared lock
int where_lists_get(pg_ctx* ctx, pg_index* ix, const WhereId& id, const RowFilter& f, std::shared_ptr<WhereLists>* out) {
    const WhereKey key = id.w ? WhereKey{id.fs, -1, 0, 0, 0, ix->gen, id.w, id.epoch}
                              : WhereKey{id.fs, id.column, id.fs->cols[(size_t)id.column].version, f.op, f.val, ix->gen, nullptr, 0};
    std::lock_guard<std::mutex> g(ix->where_mu);
    return where_cache_get(ix->where_cache, ix->where_st, ctx->knobs.index_where_cache, key, out, [&](std::shared_ptr<WhereLists>* built) {
        const int rc = where_lists_build(ctx, ix, f, built);
        if (rc == PG_ERR_DEVICE) set_error("index filtered lists: %s", hipGetErrorString(hipGetLastError()));
        else if (rc) set_error("index filtered lists: device allocation failed (%llu rows)", (unsigned long long)ix->rows);
        return rc;
    });
}

}  // namespace pg

extern "C" {

int pg_index_where_read(pg_ctx* ctx, const pg_index* ixc, const pg_features* fs, int column, int op, long long value, uint32_t* offsets,
                        uint32_t* perm, uint64_t* admitted) {
    PG_REQUIRE(ctx && ixc && fs, "pg_index_where_read: NULL argument");
    PG_REQUIRE(column >= 0 && (size_t)column < fs->cols.size(), "pg_index_where_read: column %d out of range", column);
    PG_REQUIRE(op >= 0 && op <= 5, "pg_index_where_read: op %d unknown (0 >, 1 >=, 2 <, 3 <=, 4 ==, 5 !=)", op);
    PG_REQUIRE(fs->rows >= ixc->rows, "pg_index_where_read: the feature store holds %llu rows, the index %llu", (unsigned long long)fs->rows,
               (unsigned long long)ixc->rows);
    const pg_features::Column& c = fs->cols[(size_t)column];
    if ((c.dtype != PG_F_I32 && c.dtype != PG_F_I64) || !c.d) {
        pg::set_error("pg_index_where_read: column \"%s\" must be an int32 / int64 column with values", c.name.c_str());
        return PG_ERR_UNSUPPORTED;
    }
    pg::RowFilter f;
    f.col = c.d;
    f.dtype = c.dtype;
    f.op = op;
    f.val = value;
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(ix->t->rw);
    std::shared_ptr<pg::WhereLists> wl;
    int rc;
    if ((rc = pg::where_lists_get(ctx, ix, pg::WhereId{fs, column, nullptr, 0}, f, &wl))) return rc;
    hipStream_t s = ctx->stream;
    if (offsets) PG_HIP(hipMemcpyAsync(offsets, wl->off, ((size_t)ix->n_lists + 1) * 4, hipMemcpyDeviceToHost, s));
    if (perm && wl->admitted) PG_HIP(hipMemcpyAsync(perm, wl->perm, (size_t)wl->admitted * 4, hipMemcpyDeviceToHost, s));
    PG_HIP(hipStreamSynchronize(s));
    if (admitted) *admitted = wl->admitted;
    return PG_OK;
}

int pg_index_where_stats(const pg_index* ixc, pg_index_where_stats_t* out) {
    PG_REQUIRE(ixc && out, "pg_index_where_stats: NULL argument");
    pg_index* ix = const_cast<pg_index*>(ixc);
    std::lock_guard<std::mutex> g(ix->where_mu);
    *out = ix->where_st;
    return PG_OK;
}

}  // extern "C"
