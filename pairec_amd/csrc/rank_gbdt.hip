// rank_gbdt.hip — PG_MODEL_GBDT: a forest of complete binary trees over a request's user features and the candidates' typed
// feature columns (the PS-SMART models behind the reference's PMML processor).  No matrix work: the cost is dependent LDS reads.
//
//     x = [ user_feats[r] | columns item_cols at cand_rows[i] ]      fp32, an item value converted once (feature_cols.hpp)
//     tree t: n = 0; d times: n = 2n + 1 if x[f_n] < thr_n, or x[f_n] is NaN and node n sends a missing value left; else 2n + 2
//     margin = (double)base + sum_t (double)leaf_t[n - (2^d - 1)]    fp64, ascending t: the specification
//     score  = (float)margin, or (float)(1 / (1 + go_exp(-margin)))
//
// Work split.  One lane owns one candidate through the whole forest, so the fp64 chain keeps tree order whatever the grid is.  A
// workgroup takes a tile of TILE candidates of ONE request (build_tiles_launch cuts the requests on the device: nothing here
// synchronises with the host): one wave, TILE = 64, so that a request of a few thousand candidates spreads over the chip; four
// waves, TILE = 256, in a call of at least kGbdtWideItems candidates, where every workgroup streams the whole forest out of L2 and
// a four times larger tile streams it a quarter as often.
//
// Feature rows.  The tile's values sit in LDS transposed, X[f][TILE] fp32, f over the user features and then the item columns.
// Lane j reads feature f at word f TILE + j: bank j for every f, so 64 lanes whose nodes name 64 different features hit 64
// different banks.  The user features are written into rows of the same pitch (one broadcast load per row) rather than into one
// short row: a node's word then turns into the address with ONE shift-add — its low 24 bits are the feature index, the
// missing-left flag sits in bits 30 and 31 where the 24-bit multiply does not look — and a visit is 7 vector instructions against
// 6 LDS issue cycles.  With a short broadcast row the address needs a compare and two selects more, and the vector pipe falls
// further behind.  The price is LDS: (n_user + n_item) TILE 4 bytes, 64 KiB for 32 + 32 features in a wide tile.
//
// Forest.  4096 trees of depth 8 are 12 MiB, so the forest streams through LDS in chunks of kGbdtChunkBytes = 24 KiB, whole
// trees only (rank_model.hpp pack_gbdt: 2^(11 - d) records of 12 << d bytes), double-buffered as rank_mmoe.hip's weight records:
// chunk c + 1 is requested into registers before chunk c is walked and stored into the other buffer after it, one barrier per
// chunk.  The device record is the blob's tree with every level reversed, so that "left" is the ODD child: the heap index m
// (root 1) moves to 2m + left, one select and one shift-or.  A visit reads the 8-byte node record { word, thr } with one
// ds_read_b64, then the feature with one ds_read_b32, then compares; the walk is branch-free with the depth a template
// parameter, so no lane diverges.  The two reads depend on each other
// and on the visit before, so a lane walks EIGHT trees of the chunk at once (a chunk holds at least eight) and adds their eight
// leaves to its fp64 accumulator in tree order afterwards; a forest's last n_tree % 8 trees go one at a time.
//
// LDS: 48 KiB of chunk buffers + the feature rows: at most 80 KiB with one wave, 128 KiB with four (kGbdtWideMaxFeat).
#include "expr_prog.hpp"
#include "feature_cols.hpp"
#include "rank_mlp.hpp"

namespace pg {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct GbdtCols { ColDesc c[kGbdtMaxFeat]; };       // the item columns' descriptors: kernel arguments, nothing staged
struct GbdtArgs {
    const uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles;
    const float* user;          // [n_req][nu]
    const uint32_t* cand;
    const char* forest;
    float* out;
    uint64_t rows;              // of the feature store
    uint32_t nu, ni, n_tree, obj;
    float base;
};

// K trees of depth D whose records start at LDS byte rec0, for the lane whose feature column starts at LDS byte xlane
template <int D, int TILE, int K>
__device__ __forceinline__ void gbdt_walk(const char* smem, uint32_t rec0, uint32_t xlane, double& acc) {
    constexpr uint32_t REC = gbdt_tree_bytes(D);
    uint32_t m[K];                                      // the device record's heap index: children 2m (right) and 2m + 1 (left)
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = 1;
#pragma unroll
    for (int s = 0; s < D; ++s) {
        uint2 nd[K];
        float x[K];
#pragma unroll
        for (int k = 0; k < K; ++k) nd[k] = *reinterpret_cast<const uint2*>(smem + (8u * m[k] + (rec0 + k * REC - 8u)));
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = *reinterpret_cast<const float*>(smem + (__umul24(nd[k].x, (uint32_t)TILE * 4u) + xlane));
#pragma unroll
        for (int k = 0; k < K; ++k) {
            // word >> 30 is the class mask sNaN | qNaN where a missing value goes left, else 0 (bitwise |: || is a divergent branch)
            const bool left = (x[k] < __uint_as_float(nd[k].y)) | __builtin_amdgcn_classf(x[k], (int)(nd[k].x >> 30));
            m[k] = 2 * m[k] + (left ? 1u : 0u);
        }
    }
    float leaf[K];
#pragma unroll
    for (int k = 0; k < K; ++k)                         // leaf slot m - 2^D behind the 2^D node slots
        leaf[k] = *reinterpret_cast<const float*>(smem + (4u * m[k] + (rec0 + k * REC + (4u << D))));
#pragma unroll
    for (int k = 0; k < K; ++k) acc += (double)leaf[k];
}

template <int D, int TILE>
__global__ __launch_bounds__(TILE) void gbdt_kernel(GbdtArgs a, GbdtCols cols) {
    extern __shared__ __attribute__((aligned(16))) char smem[];     // two chunk buffers, then X[nu + ni][TILE]
    constexpr uint32_t CHUNK = kGbdtChunkBytes, REC = gbdt_tree_bytes(D), TPC = gbdt_chunk_trees(D);
    constexpr int NLD = CHUNK / 16 / TILE;              // 16-byte loads per thread and chunk
    static_assert(TPC >= 8 && TPC % 8 == 0 && NLD * 16 * TILE == (int)CHUNK, "chunk");
    const uint32_t tile = blockIdx.x;
    if (tile >= *a.n_tiles) return;
    const uint32_t tid = threadIdx.x, req = a.tile_req[tile], item0 = a.tile_item0[tile];
    const bool live = tid < a.tile_cnt[tile];
    const uint32_t n_chunk = (a.n_tree + TPC - 1) / TPC;            // (the device copy holds whole chunks)

    u32x4 st[NLD];
    auto request = [&](uint32_t c) {
        const u32x4* const g = reinterpret_cast<const u32x4*>(a.forest + (size_t)c * CHUNK);
#pragma unroll
        for (int i = 0; i < NLD; ++i) st[i] = g[i * TILE + tid];
    };
    auto deliver = [&](uint32_t buf) {
        u32x4* const l = reinterpret_cast<u32x4*>(smem + buf * CHUNK);
#pragma unroll
        for (int i = 0; i < NLD; ++i) l[i * TILE + tid] = st[i];
    };
    request(0);

    // the tile's feature rows: user features (the same value in every lane's column), then the item columns at the lane's row
    float* const X = reinterpret_cast<float*>(smem + 2 * CHUNK);
    for (uint32_t f = 0; f < a.nu; ++f) X[f * TILE + tid] = a.user[(size_t)req * a.nu + f];
    const uint32_t row = live ? a.cand[item0 + tid] : 0u;
    for (uint32_t f0 = 0; f0 < a.ni; f0 += 4) {         // four columns' loads in flight
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (live && f0 + u < a.ni) ? load_as_f32(cols.c[f0 + u], row, a.rows) : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (f0 + u < a.ni) X[(a.nu + f0 + u) * TILE + tid] = v[u];
    }
    deliver(0);
    __syncthreads();

    const uint32_t xlane = 2 * CHUNK + 4 * tid;
    double acc = (double)a.base;
    for (uint32_t c = 0; c < n_chunk; ++c) {
        const bool more = c + 1 < n_chunk;              // (uniform: every thread meets every barrier)
        if (more) request(c + 1);
        const uint32_t nt = a.n_tree - c * TPC < TPC ? a.n_tree - c * TPC : TPC, rec0 = (c & 1) * CHUNK;
        uint32_t t = 0;
        for (; t + 8 <= nt; t += 8) gbdt_walk<D, TILE, 8>(smem, rec0 + t * REC, xlane, acc);
        for (; t < nt; ++t) gbdt_walk<D, TILE, 1>(smem, rec0 + t * REC, xlane, acc);
        if (more) deliver((c + 1) & 1);
        __syncthreads();
    }
    if (live) a.out[item0 + tid] = a.obj ? (float)acc : (float)(1.0 / (1.0 + go_exp(-acc)));
}

template <int D, int TILE>
static int launch_gbdt(pg_ctx* ctx, const GbdtArgs& a, const GbdtCols& cols, uint32_t grid) {
    const size_t lds = 2 * (size_t)kGbdtChunkBytes + (size_t)(a.nu + a.ni) * TILE * 4;
    int rc;
    if ((rc = ensure_dyn_lds(ctx, (const void*)gbdt_kernel<D, TILE>, lds))) return rc;
    gbdt_kernel<D, TILE><<<grid, TILE, lds, ctx->stream>>>(a, cols);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
template <int TILE>
static int launch_gbdt_depth(pg_ctx* ctx, uint32_t depth, const GbdtArgs& a, const GbdtCols& cols, uint32_t grid) {
    switch (depth) {
        case 1: return launch_gbdt<1, TILE>(ctx, a, cols, grid);
        case 2: return launch_gbdt<2, TILE>(ctx, a, cols, grid);
        case 3: return launch_gbdt<3, TILE>(ctx, a, cols, grid);
        case 4: return launch_gbdt<4, TILE>(ctx, a, cols, grid);
        case 5: return launch_gbdt<5, TILE>(ctx, a, cols, grid);
        case 6: return launch_gbdt<6, TILE>(ctx, a, cols, grid);
        case 7: return launch_gbdt<7, TILE>(ctx, a, cols, grid);
        default: return launch_gbdt<8, TILE>(ctx, a, cols, grid);
    }
}

int rank_gbdt_dev_locked(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_cols, const float* d_user,
                         const uint32_t* d_cand, const uint32_t* d_off, uint32_t n_req, uint32_t n_items, float* d_out) {
    if (n_items == 0 || n_req == 0) return PG_OK;
    const bool wide = n_items >= kGbdtWideItems && m->gb_nu + m->gb_ni <= kGbdtWideMaxFeat;
    const uint32_t tile = wide ? kGbdtWideTile : kGbdtTile, max_tiles = n_items / tile + n_req;
    uint32_t *tile_req, *tile_item0, *tile_cnt, *n_tiles, *req_tile0;
    int rc;
    if ((rc = scratch_carve(ctx, kSlotGbdt, [&](Carve& c) {
            tile_req = c.take<uint32_t>(max_tiles);
            tile_item0 = c.take<uint32_t>(max_tiles);
            tile_cnt = c.take<uint32_t>(max_tiles);
            n_tiles = c.take<uint32_t>(64);
            req_tile0 = c.take<uint32_t>(n_req);
        }))) return rc;
    GbdtCols cols;
    memset(&cols, 0, sizeof cols);
    for (uint32_t f = 0; f < m->gb_ni; ++f) {
        const auto& c = fs->cols[(size_t)item_cols[f]];
        cols.c[f] = ColDesc{c.d, c.dtype, 0, c.def};
    }
    const bool timed = !ctx->timers_off;
    if (timed) PG_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((rc = build_tiles_launch(ctx, d_off, n_req, max_tiles, tile, tile_req, tile_item0, tile_cnt, n_tiles, req_tile0))) return rc;
    GbdtArgs a{};
    a.tile_req = tile_req;
    a.tile_item0 = tile_item0;
    a.tile_cnt = tile_cnt;
    a.n_tiles = n_tiles;
    a.user = d_user;
    a.cand = d_cand;
    a.forest = (const char*)m->gb_forest;
    a.out = d_out;
    a.rows = fs->rows;
    a.nu = m->gb_nu;
    a.ni = m->gb_ni;
    a.n_tree = m->gb_ntree;
    a.obj = m->gb_obj;
    a.base = m->gb_base;
    rc = wide ? launch_gbdt_depth<(int)kGbdtWideTile>(ctx, m->gb_depth, a, cols, max_tiles)
              : launch_gbdt_depth<(int)kGbdtTile>(ctx, m->gb_depth, a, cols, max_tiles);
    if (rc) return rc;
    if (timed) {
        PG_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->rank_timing_pending = true;
    }
    return PG_OK;
}

}  // namespace pg
