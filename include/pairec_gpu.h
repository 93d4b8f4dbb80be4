/*
 * pairec_gpu.h — C ABI of libpairec_gpu.so, the MI355X (gfx950) engine behind pairec's
 * rank + recall hot path.
 *
 * This is the drop-in boundary: every entry point replaces one network hop of the reference
 * (alibaba/pairec, Go).  A cgo shim implements algorithm.IAlgorithm,
 * recall.Recall and sort.ISort on top of these calls.  Signatures use plain pointers and sizes;
 * no C++ or torch types cross the boundary.
 *
 * Conventions
 *   - every function returns 0 on success, a negative pg_status on failure; pg_last_error()
 *     returns a thread-local message.  Nothing throws or aborts across the ABI (the reference's
 *     rank goroutines have no recover(), service/rank/rank_service.go:265-288).
 *   - all entry points are re-entrant: the reference calls IAlgorithm.Run concurrently from one
 *     goroutine per batch × per algo (rank_service.go:264-289).  Calls on one pg_ctx are serialised
 *     on that context's HIP stream.
 *   - "_dev" variants take device pointers (HBM-resident inputs/outputs, used to chain stages and
 *     by bench.py); the plain variants take host pointers (what the cgo shim passes) and copy.
 *   - row ids are uint32 table row indices (+ a uint64 per-table row_offset for sharded tables);
 *     item-id strings stay on the host side (module.ItemId is a string, module/item.go:13).
 */
#ifndef PAIREC_GPU_H
#define PAIREC_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pg_ctx pg_ctx;
typedef struct pg_table pg_table;      /* HBM-resident embedding table  (module.VectorDao backend) */
typedef struct pg_model pg_model;      /* rank model weights            (algorithm/eas model)      */
typedef struct pg_expr pg_expr;        /* compiled RankScore expression (utils/ast)                */
typedef struct pg_where pg_where;      /* compiled compound WhereClause (HologresVectorConf.WhereClause) */

typedef enum {
    PG_OK = 0,
    PG_ERR_INVALID = -1,     /* bad argument */
    PG_ERR_DEVICE = -2,      /* HIP runtime error (message carries hipGetErrorString) */
    PG_ERR_NOMEM = -3,
    PG_ERR_UNSUPPORTED = -4, /* shape outside what the kernels are built for */
    PG_ERR_ARITH = -5,       /* expression: division by zero / modulo by zero (reference panics) */
    PG_ERR_PARSE = -6,       /* expression: lexer "symbol error" (utils/ast/parse.go:125-133) */
    PG_ERR_EMPTY = -8,       /* pg_table_view_create: no row passes the filter (a result, not a misconfiguration) */
    PG_ERR_TIMEOUT = -7      /* the call's deadline passed (algorithm/eas/client.go:53-58: 100 ms default per predict); the
                                work it belonged to still completes for the other callers of its batch */
} pg_status;

/* Precision of a rank model's two matrix layers.  The reference hands model outputs on as fp32 widened to f64
 * (algorithm/eas/easyrec_response.go:479-483, eas/tf_response.go:55-59).
 *   PG_PREC_F32    fp32 MFMA, bit-defined (a k-ordered fmaf chain): the specification.
 *   PG_PREC_BF16   operands rounded to bf16, fp32 accumulation: fastest; scores within ~4e-5 of the fp32 path.
 *   PG_PREC_BF16X3 "split bf16": every operand as hi + lo bf16, three products per term into the fp32 accumulator, nothing
 *                  else rounded: scores within 1e-5 of PG_PREC_F32 (observed ~1e-6) at the bf16 matrix pipe's speed / 3.
 *   PG_PREC_F16X2  PG_MODEL_DNN3[_MULTI] only.  Activations rounded once to fp16 (RNE), weights as hi + lo fp16, two products
 *                  per term into the fp32 accumulator.
 *   PG_PREC_F16    the same with the weights rounded once too: one product per term.
 *                  Both carry PG_PREC_BF16X3's contract — scores within 1e-5 of PG_PREC_F32 — and keep it by range
 *                  handling, not by luck.  Scaling rule (every factor an exact power of two, fixed at pg_model_load): with
 *                  E_k = floor(log2 max_j |W1[k][j]|) per item input column and F_i = floor(log2 max_j |W2[i][j]|) per
 *                  hidden unit (0 for an all-zero row), the kernel converts x_k * 2^(E_k + G) and relu(z1_i) * 2^(F_i + G)
 *                  to fp16 against weights scaled by 2^(-E_k - G + S) and 2^(-F_i - G + S); G = 11, S = 23 (undone
 *                  exactly where the accumulators are read).  A scaled activation that underflows fp16's normal range
 *                  costs at most 2^-24 per term in units where the weight row's maximum is in [1, 2), i.e. at most
 *                  fan_in * 2^-24 per pre-activation; one that overflows (a single term of order 2^5 in those units), or
 *                  is not finite, sends its 128-item tile to the PG_PREC_BF16X3 kernel, enqueued behind the fp16 one — the
 *                  tile's scores are then exactly a PG_PREC_BF16X3 model's.  A call the fp16 kernel does not cover
 *                  (hidden widths 1024-512, a table of dim != 128, the rank_no_ws option) is served whole by the
 *                  PG_PREC_BF16X3 path, bit for bit.  Never an error, never a silently worse score; pg_model_f16_stats counts.
 *                  Refused at load (PG_ERR_UNSUPPORTED): PG_MODEL_FM_TWOTOWER; a non-finite weight; a scaled weight or
 *                  scale factor outside fp32's normal range. */
typedef enum { PG_PREC_F32 = 0, PG_PREC_BF16 = 1, PG_PREC_BF16X3 = 2, PG_PREC_F16X2 = 3, PG_PREC_F16 = 4 } pg_prec;
typedef enum { PG_MODEL_DNN3 = 1, PG_MODEL_FM_TWOTOWER = 2, PG_MODEL_DNN3_MULTI = 3 } pg_model_kind;

const char* pg_last_error(void);
const char* pg_version(void);

/* ---- context --------------------------------------------------------------------------------
 * One context = one GPU + one HIP stream.  `stream` may be an existing hipStream_t (e.g. a dedicated stream
 * torch.distributed's collectives are ordered on) or NULL to create a private one.  The null stream (handle 0,
 * torch's default stream) cannot be adopted — NULL always means "private": a host that mixes its own device work
 * with library calls creates a stream of its own and passes it here (pairec_amd/dist.py shard_context). */
/* gfx950 devices this process can see (what a host sizes pg_group_create / its replica list with; the reference has no
 * counterpart — its FAISS / EAS endpoints are URLs in recconf, algorithm/eas/model.go:38-60). */
int pg_device_count(int* out);
int pg_init(int device, void* stream, pg_ctx** out);
int pg_shutdown(pg_ctx* ctx);
int pg_synchronize(pg_ctx* ctx);
/* Developer / test knobs of one context (defaults come from PG_* environment variables read once, in pg_init):
 * "no_pilot", "recall_exact", "screen_min", "pilot_fraction", "chunk_growth", "seed_rows", "pilot_growth",
 * "pilot_sigmas", "debug_scan", "rank_no_ws", and for the 4-bit screen of batches of <= 4 queries
 * (csrc/recall_i4.hip) "no_screen_i4", "i4_min_rows" (default 2^22), "i4_max_lambda", and for the threshold refinement inside the pilot plan's
 * full pass "no_refine", "refine_min_rows" (default 2^24), and for the threshold model that replaces the pilot sample
 * once a table has seen >= 1024 queries of one K (plan 0) "no_predict", "predict_sigmas" (default 4.5),
 * "predict_min_rows" (default 2^22), and for the 256-query screen "screen_early_share" (default 604: the share
 * x 1024 of a SIMD's blocks its older wave takes; 512 = even), "screen_early_share_narrow" (the <= 128-query kernels, default
 * 512); for the squared-Euclidean recall "l2_exact", "l2_max_slack" (default 1.0); for pg_recall_topk_where the compact route's
 * limits "where_compact_max_rows" (default 2^23; half of it for batches of <= 4 queries) and "where_compact_min_ratio"
 * (default 8: at most an eighth of the table); round 6: for the 1 … 64-query passes on the 4-bit shadow through the matrix pipe
 * (csrc/recall_i4m.hip) "no_screen_i4m", "i4m_min_queries" (default 1), "i4m_max_queries" (64), "i4m_max_lambda", "i4m_max_pairs";
 * for crowded tables "max_rec_scale", "no_r2", "r2_min_factor", "predict_max_factor"; for the coalescer "coalescer_rejoin",
 * "coalescer_rejoin_us_per_caller"; and which sort a call with few lists takes (csrc/split_sort.hpp): "rank_sort_max" (default 32
 * lists) with "rank_sort_work" (lists x items^2 <= 7e7: counting ranks), "split_sort_max" (default 96 lists of 1025 … 8192 items:
 * runs sorted wave by wave over the chip; 0 = never); "stage_timers" (default 1; 0: this context's direct calls record no HIP events
 * around the recall plan, its scan launches and the rank stage — pg_stats' last_*_ms and pg_last_scan_kernel_ms stop moving, a
 * small batch's step gets 40-60 us shorter; a coalescer's batches never record them, see there); for recalls through a pg_index
 * "index_dense_fraction" (default 0.01: a batch of nq queries whose live (row, query) pairs exceed this x rows x nq^0.6 takes
 * the table's pass), and for an attached index "index_plan_rounds" / "index_skip_batches" (see pg_index_attach); for filtered
 * recalls through an index (pg_index_recall_topk_where) "index_where_cache" (default 4 filtered lists kept per index; 0 = built
 * per call and freed after it) and "index_route_where" (default 0; 1: pg_recall_topk_where on a table whose attached index is
 * current searches that index, synchronously); for pg_index_refresh "index_refresh_full_fraction" (default 0.1: in auto mode
 * more written rows than this share of the table are refreshed in full; a table's write log is dropped past it too); for
 * coalescers created afterwards "coalescer_max_exclude" (default 0, 0..4096: the longest list pg_coalescer_recall_exclude takes;
 * a value outside the range is PG_ERR_INVALID); for pg_cf_recall "cf_lds_max_pairs" (default and largest value 6144: a request
 * of at most this many (trigger, neighbour) pairs keeps its table in LDS, a larger one in global memory; 0 = always global;
 * pg_x2i_recall reads the same knob for its (X, item) pairs and cuts it to 5120, what its smaller LDS table serves);
 * for pg_fanin_merge_dev "fanin_lds_max_cap" (default and largest value 8192 = PG_FANIN_LDS_MAX_CAP: a merge of at most this
 * many candidates per request keeps its table in LDS, a larger one in context scratch; 0 = always scratch).
 * value is parsed as a number. */
int pg_set_option(pg_ctx* ctx, const char* name, const char* value);
int pg_device_malloc(pg_ctx* ctx, size_t bytes, void** out);
int pg_device_free(pg_ctx* ctx, void* p);
int pg_memcpy_h2d(pg_ctx* ctx, void* dst, const void* src, size_t bytes);
int pg_memcpy_d2h(pg_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- embedding tables -----------------------------------------------------------------------
 * Replaces module.VectorDao.VectorString (module/vector_dao.go:13-15) and its six remote
 * back-ends: rows live in HBM as row-major fp32 [rows][dim].  dim must be a multiple of 64. */
int pg_table_create(pg_ctx* ctx, uint64_t rows, uint32_t dim, uint64_t row_offset, pg_table** out);
int pg_table_destroy(pg_ctx* ctx, pg_table* t);
/* deterministic synthetic fill: global row = row_offset + local row */
int pg_table_fill_synthetic(pg_ctx* ctx, pg_table* t, uint64_t seed, int normalize);
/* i.i.d. N(0, sigma^2) elements, unnormalised rows — the second benchmark distribution (trained embeddings look
 * Gaussian; the uniform rows of SURVEY.md 8d are the int8 screen's best case).  Defined by the device's own fp64
 * log / cos: reproducible run to run, compared in tests against downloaded rows. */
int pg_table_fill_gaussian(pg_ctx* ctx, pg_table* t, uint64_t seed, float sigma);
/* clustered rows — the third benchmark distribution (trained embeddings cluster: the tables behind
 * service/recall/hologres_vector_recall.go:23): n_centres centres on the unit sphere, a row = its centre + noise of norm
 * ~ sigma, normalised.  No transcendental in it: oracle/oracle.c regenerates any slice bit for bit. */
int pg_table_fill_mixture(pg_ctx* ctx, pg_table* t, uint64_t seed, uint32_t n_centres, float sigma);
int pg_table_upload(pg_ctx* ctx, pg_table* t, uint64_t row0, uint64_t nrows, const float* host_rows);
int pg_table_download(pg_ctx* ctx, const pg_table* t, uint64_t row0, uint64_t nrows, float* host_rows);
/* atomically exchange the contents of two tables of equal shape (the analogue of the Hologres
 * partition hot-swap, module/vector_hologres_dao.go:40-61) */
int pg_table_swap(pg_ctx* ctx, pg_table* a, pg_table* b);
int pg_table_info(const pg_table* t, uint64_t* rows, uint32_t* dim, uint64_t* row_offset);
/* embedding lookup by row (the VectorString analogue): out[n][dim] fp32 */
int pg_table_gather(pg_ctx* ctx, const pg_table* t, const uint32_t* rows, uint32_t n, float* out);

/* ---- recall: exact inner-product top-K ------------------------------------------------------
 * Replaces FaissModel.Run → VectorClient.Search (algorithm/faiss/model.go:29-31,
 * vector_client.go:32-41; VectorRequest{k, vector} → VectorReply{retval, scores},
 * vectorretrieval.proto:11-20) and the Hologres pm_approx_inner_product_distance ORDER BY desc
 * LIMIT n query (service/recall/hologres_vector_recall.go:23).
 *   score(row) = chain_k fmaf(x[row][k], q[k], acc)  (k ascending, fp32) — independent of nq.
 *   order: score descending (IEEE totalOrder, NaN last), then row ascending.
 * queries: [nq][dim] fp32, nq <= 256 per call (<= 32 when dim > 128); one call = one table pass.
 * Finite tables of dim 128 / 64 are scanned with an int8 / bf16 MFMA screen over a quantised shadow of the rows
 * (a rigorous bound of every score) followed by exact re-scoring of the survivors, everything else with the
 * exact fp32-MFMA scan (groups of 64 queries per launch) — results are identical bit for bit.  out_rows: [nq][k] global row ids (row_offset + local), out_scores:
 * [nq][k].  If the table has fewer than k rows the tail is filled with
 * row = UINT64_MAX, score = -inf and *out_count (optional) receives the valid count. */
int pg_recall_topk(pg_ctx* ctx, const pg_table* t, const float* queries, uint32_t nq, uint32_t k,
                   uint64_t* out_rows, float* out_scores, uint32_t* out_count);
int pg_recall_topk_dev(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq,
                       uint32_t k, uint64_t* d_out_rows, float* d_out_scores, uint32_t* out_count);
/* HologresVectorRecallV2 (service/recall/hologres_vector_recall_v2.go:23,96-206): the k rows of SMALLEST squared Euclidean
 * distance to each query, ascending, the distance as the item's score (:181-189).  Exact (the reference's Proxima index is
 * approximate): d = fmaf(-2, ip, |x|^2 + |q|^2), each sum a k-ascending fp32 fmaf chain; ties by row ascending; slots beyond
 * the table's rows carry row UINT64_MAX and distance +inf.  dim 64 or 128.  A dim-128 table with an int8 shadow is served from
 * it — one integer cutoff per 32-row block where the rows have (nearly) one norm, a per-row test otherwise (knob "l2_max_slack");
 * suspects are re-scored exactly — any other table (and knob "l2_exact") by the exact scan over the fp32 rows. */
int pg_recall_topk_l2(pg_ctx* ctx, const pg_table* t, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                      float* out_dist, uint32_t* out_count);
int pg_recall_topk_l2_dev(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                          float* d_out_dist, uint32_t* out_count);
/* I2IVectorRecall.GetCandidateItems (service/recall/item_2_item_vector_racall.go:51-152): the embeddings of the
 * trigger items (context parameter "item_id" → dao.VectorString) are the queries — rows `trigger_rows[n]` of
 * `trigger_table` (same dim as `t`; usually the same table) against `t`.  Outputs as pg_recall_topk; the trigger
 * item itself is not excluded (neither does the reference's SQL). */
int pg_i2i_recall(pg_ctx* ctx, const pg_table* trigger_table, const uint32_t* trigger_rows, uint32_t n,
                  const pg_table* t, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count);
/* OnlineVectorRecall.GetCandidateItems (service/recall/online_vector_recall.go:73-155): user features → the vector
 * model's user embedding → its FaissNeighNum = k nearest items (TorchrecEmbeddingItemsResponse: match_item_scores +
 * item_ids, algorithm/eas/easyrec_response.go:700-734).  `m` is a PG_MODEL_FM_TWOTOWER whose user tower produces the
 * embedding (pg_fm2t_user_embedding), `item_emb` the item-tower outputs as a table of dim t_out. */
int pg_online_vector_recall(pg_ctx* ctx, const pg_model* m, const pg_table* item_emb, const float* user_vecs,
                            uint32_t n_req, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count);
/* merge `nlists` sorted/unsorted (row,score) lists of `per_list` entries per query into the global
 * top-k (multi-GPU: the lists are the all-gathered per-shard results).  Layout [nq][nlists][per_list]. */
int pg_topk_merge_dev(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq,
                      uint32_t nlists, uint32_t per_list, uint32_t k, uint64_t* d_out_rows,
                      float* d_out_scores);

/* global row ids (as returned by recall/merge) → local row indices of table `t` for the rank stage;
 * d_owned (optional, uint8 per entry) receives 1 where the row lives in this shard, else 0 and
 * the local index is written as 0.  UINT64_MAX padding is "not owned". */
int pg_rows_to_local_dev(pg_ctx* ctx, const pg_table* t, const uint64_t* d_rows, uint32_t n,
                         uint32_t* d_local, uint8_t* d_owned);

/* ---- rank: model predict --------------------------------------------------------------------
 * Replaces EasModel.Run / TFservingModel.Run (algorithm/eas/model.go:197-222,
 * algorithm/tfserving/model.go:30-55): the DNN / FM forward that the reference ships to a
 * remote PAI-EAS / TF-Serving process, one call per batch of BatchCount=100 items
 * (service/rank/rank_service.go:163-166).  Here one call scores any number of requests.
 *
 * PG_MODEL_DNN3 blob (little-endian fp32 unless noted):
 *   u32 d_user, d_item, h1, h2;  w1[(d_user+d_item)][h1]; b1[h1]; w2[h1][h2]; b2[h2]; w3[h2]; b3
 *   score = sigmoid( w3 · relu( W2ᵀ relu( W1ᵀ [user ‖ item_row] + b1 ) + b2 ) + b3 )
 *   shapes: d_user 1..4096; d_item 64 or 128 (= the table's dim); (h1, h2) in {128-128, 256-128, 256-256, 512-256,
 *   1024-512}; the benchmark shape [128+128]-512-256 in bf16 runs on the weights-stationary kernel
 * PG_MODEL_DNN3_MULTI blob — a multi-output model: n_out heads on ONE shared trunk, the shape of the reference's own fixtures
 * (EasyrecResponse.multiValModule, algorithm/eas/easyrec_response.go:35-70: probs_ctr / probs_cvr of one PAI-EAS model;
 * RankService writes them as "<algo>_<output>", service/rank/rank_service.go:315-319):
 *   u32 d_user, d_item, h1, h2, n_out (1..8);  w1; b1; w2; b2 as above; w3[h2][n_out]; b3[n_out]
 *   score_o = sigmoid( w3[:, o] · h2 + b3[o] ) — every head has exactly the arithmetic of a PG_MODEL_DNN3 with that column
 *   (in PG_PREC_F32, bit for bit); ONE gather and ONE trunk per item whatever n_out.  pg_model_load stores it as a
 *   PG_MODEL_DNN3 with pg_model_num_outputs() = n_out: pg_rank_dnn3[_dev] then write n_out planes, out_scores[o * n_items + i]
 *   (n_items = req_offsets[n_req], resp. the n_items argument), and pg_coalescer_rank_dnn3 n_out planes of its n candidates.
 * Exported weights: every matrix is plain row-major [in][out] fp32 exactly as a Dense layer's kernel is saved;
 * tools/pack_model.py builds either blob from an .npz of such arrays.
 * PG_MODEL_FM_TWOTOWER blob:
 *   u32 n_user_fields, n_item_fields, k, d_user, t_h1, t_out, vocab; f32 fm_b;
 *   uw1[d_user][t_h1]; ub1; uw2[t_h1][t_out]; ub2; iw1[nif*k][t_h1]; ib1; iw2[t_h1][t_out]; ib2;
 *   then per field f (user fields first): emb_f[vocab][k], lin_f[vocab]
 *   score = sigmoid( y_fm + <user_tower(user), item_tower(concat item field embeddings)> )
 *   shapes: 1..16 user fields; n_item_fields x k = 128 with k in {8, 16, 32}; towers (t_h1, t_out, k) in
 *   {256-64 k16, 256-64 k32, 128-64 k8, 512-128 k16}
 * Summation orders are specified in DESIGN.md §5 (they are what makes PG_PREC_F32 bit-reproducible).
 */
int pg_model_load(pg_ctx* ctx, pg_model_kind kind, pg_prec prec, const void* blob, size_t len,
                  pg_model** out);
int pg_model_destroy(pg_ctx* ctx, pg_model* m);
/* outputs per item: 1, or n_out of a PG_MODEL_DNN3_MULTI */
int pg_model_num_outputs(const pg_model* m, uint32_t* out);
/* PG_PREC_F16X2 / PG_PREC_F16 models: out = {rank calls, 128-item tiles the fp16 kernel took, tiles of those re-served by the
 * PG_PREC_BF16X3 kernel (out of range / non-finite data), calls served whole by the PG_PREC_BF16X3 path}.  Zeros for a model
 * of another precision.  Waits for the model's context to drain (the tile counts live on the device; nothing on the rank
 * path reads them back). */
int pg_model_f16_stats(const pg_model* m, uint64_t out[4]);

/* DNN3: R requests; request r has user vector user_vecs[r][d_user] and candidates
 * cand_rows[req_offsets[r] .. req_offsets[r+1]) (local row indices into `t`).  out_scores is fp32
 * per candidate, request order preserved (response.AlgoResponse order contract,
 * rank_service.go:312-335). */
int pg_rank_dnn3(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* user_vecs,
                 const uint32_t* cand_rows, const uint32_t* req_offsets, uint32_t n_req,
                 float* out_scores);
int pg_rank_dnn3_dev(pg_ctx* ctx, const pg_model* m, const pg_table* t, const float* d_user_vecs,
                     const uint32_t* d_cand_rows, const uint32_t* d_req_offsets, uint32_t n_req,
                     uint32_t n_items, float* d_out_scores);
/* FM + two-tower: user_field_ids [n_req][n_user_fields], item_field_ids [n_items][n_item_fields] */
int pg_rank_fm2t(pg_ctx* ctx, const pg_model* m, const float* user_vecs,
                 const int32_t* user_field_ids, const int32_t* item_field_ids,
                 const uint32_t* req_offsets, uint32_t n_req, float* out_scores);
int pg_rank_fm2t_dev(pg_ctx* ctx, const pg_model* m, const float* d_user_vecs,
                     const int32_t* d_user_field_ids, const int32_t* d_item_field_ids,
                     const uint32_t* d_req_offsets, uint32_t n_req, uint32_t n_items,
                     float* d_out_scores);

/* user-tower output of the two-tower model: out [n_req][t_out] = uw2' relu(uw1' P(u) + ub1) + ub2 —
 * the user embedding of online_vector_recall.go:97-109 / embedding_service.go:127 */
int pg_fm2t_user_embedding(pg_ctx* ctx, const pg_model* m, const float* user_vecs, uint32_t n_req, float* out);
int pg_fm2t_user_embedding_dev(pg_ctx* ctx, const pg_model* m, const float* d_user_vecs, uint32_t n_req, float* d_out);

/* ---- rank: score fusion (RankConfig.RankScore) ----------------------------------------------
 * Replaces ast.GetExpAST + ExprASTResult (utils/ast/ast.go:215-268,368-389): compile once,
 * evaluate per item in fp64 on the device.  Variables are bound by position: pg_expr_var_name(i)
 * names column i of `vars` ([n_vars][n_items] fp64, column-major per variable). */
int pg_expr_compile(const char* source, pg_expr** out);
int pg_expr_free(pg_expr* e);
int pg_expr_num_vars(const pg_expr* e);
/* GetExpASTWithType (utils/ast/ast.go:338-343): ast_type NULL, "" or anything but "antlr" = pg_expr_compile.  "antlr" selects the
 * reference's second evaluator (go-antlr-valuate v0.0.4, un-vendored); the engine serves the SUBSET its tests pin
 * (utils/ast/ast_test.go:30-56,90-167,213-300): + - * / ^ (^ = math.Pow, above * /, above + -), parentheses, unary minus,
 * numbers, ${name}, maxIndex(${list}) / maxValue(${list}) (antlr_functions.go:34-66) — `/` is float division (no panic).
 * Everything else returns PG_ERR_UNSUPPORTED naming the construct.  A list function becomes a variable called
 * "maxIndex(name)" / "maxValue(name)" (pg_expr_var_name) that the caller fills per item from the list property.
 * ExprASTResultByAntlr's error rule — an item that lacks ANY variable of the expression scores 0 (ast.go:374-383) — is the
 * caller's to apply (pg_expr_is_antlr tells it to). */
int pg_expr_compile_typed(const char* source, const char* ast_type, pg_expr** out);
/* The arithmetic subset of govaluate that BoostScoreSort expressions use (sort/boost_score_sort.go:20-36,
 * NewEvaluableExpressionWithFunctions with utils.GovaluateFunctions), compiled to the same program: float64 literals (digits and
 * '.'), bare and [bracketed] names, + - * / % **, unary minus, parentheses, round(x) = math.Round and round(x, n) =
 * math.Trunc(x * Pow(10, n)) / Pow(10, n) (utils/govaluate_functions.go:63-75).  Every number is a float64; `/` is Go's float
 * division (±Inf / NaN, no error); `%` is math.Mod; `**` is math.Pow as the `^` of the default grammar states it; precedence
 * + -  <  * / %  <  **  <  prefix minus (so -a ** 2 is (-a) ** 2), as the feature normalizer's govaluate evaluator has it.
 * Refused by name (PG_ERR_UNSUPPORTED): comparators, the ternary, && ||, ! ~ and the bitwise operators, strings, booleans,
 * accessors, arrays, a chained **, every other function.  "" compiles to the empty expression.
 * pg_expr_eval_host evaluates any compiled expression on host arrays (vars [n_vars][n_items], as pg_expr_eval): the program's
 * host statement, no context, no device; PG_ERR_ARITH as pg_expr_eval. */
int pg_expr_compile_govaluate(const char* source, pg_expr** out);
int pg_expr_eval_host(const pg_expr* e, const double* vars, uint32_t n_items, double* out_scores);
int pg_expr_is_antlr(const pg_expr* e);
/* RankConfig.ScoreRewrite (recconf/recconf.go:743; service/rank/rank_service.go:296-306,343-353): a map source → expression.
 * Per item the reference evaluates EVERY source's expression over the item as the algorithms left it, collects the results
 * in a map, writes them back with Item.AddAlgoScores (overwriting / adding algorithm scores named `source`) and only then
 * evaluates RankScore.  Attach the scene's rewrites to its compiled RankScore; every pipeline that fuses scores with that
 * expression (pg_recommend_*, the scene / group coalescers, pg_group_*) then evaluates them first, on the device, in f64:
 * a RankScore variable naming a source reads the rewritten score, a rewrite's own variables read the un-rewritten ones
 * (the scene's "<algo>" / "<algo>_<output>" planes and current_score).  exprs[i] == NULL: the source's expression did not
 * compile — the reference logs it and scores 0 (rank_service.go:299-303,349-351).  The expressions are copied.
 * pg_expr_eval[_dev] evaluate the bare expression over caller-made variables and know nothing of rewrites.  n = 0 removes.
 * ATTACH BEFORE CREATING ANY PIPELINE FROM THE EXPRESSION: a coalescer (for its lifetime) and a batch begun and not yet ended
 * hold variable bindings sized for the rewrites present when they were made — while there is such a holder the call fails
 * with PG_ERR_INVALID and changes nothing. */
int pg_expr_set_score_rewrites(pg_expr* rank_score, uint32_t n, const char* const* sources, const pg_expr* const* exprs);
const char* pg_expr_var_name(const pg_expr* e, int i);
int pg_expr_eval(pg_ctx* ctx, const pg_expr* e, const double* vars, uint32_t n_items,
                 double* out_scores);
int pg_expr_eval_dev(pg_ctx* ctx, const pg_expr* e, const double* d_vars, uint32_t n_items,
                     double* d_out_scores);

/* float32 model outputs → float64 AlgoResponse scores, the widening every response decoder of
 * the reference performs (algorithm/eas/easyrec_response.go:479-483, eas/tf_response.go:55-59,
 * tfserving/response.go:51-64; recall: vector_recall.go:98). */
int pg_widen_f32_dev(pg_ctx* ctx, const float* d_in, uint32_t n, double* d_out);

/* The fusion step of RankService.Rank (service/rank/rank_service.go:339-363) alone, for a host that runs the stages itself
 * (pairec_amd/dist.py's sharded step between its collectives): n items, n_planes model-score planes d_rank[p * rank_stride + i]
 * (float32, widened as the decoders do) named plane_names[p] ("<algo>" or "<algo>_<output>"), d_recall[i] = Item.Score
 * ("current_score").  RankConfig.ScoreRewrite attached to `rank_score` (pg_expr_set_score_rewrites) is evaluated first, from
 * the un-rewritten planes (rank_service.go:343-353).  d_fused[i] = the RankScore, f64.  A division by zero anywhere is
 * PG_ERR_ARITH (the call synchronises to learn it); a variable that names neither a plane, a rewrite source nor
 * current_score PG_ERR_INVALID. */
int pg_fuse_scores_dev(pg_ctx* ctx, const pg_expr* rank_score, const char* const* plane_names, uint32_t n_planes,
                       const float* d_rank, size_t rank_stride, const float* d_recall, uint32_t n, double* d_fused);

/* ---- sort -----------------------------------------------------------------------------------
 * Replaces ItemRankScoreSort (descending, sort/item_rank_score.go:26-32) and ItemScoreSort
 * (ascending, sort/item_score.go:36-41): out_order[i] = index of the i-th item.  Segmented:
 * seg_offsets[n_seg+1] delimits independent requests.  Ties keep input order; NaN last. */
int pg_sort_scores(pg_ctx* ctx, const double* scores, const uint32_t* seg_offsets, uint32_t n_seg,
                   int descending, uint32_t* out_order);
/* max_segment: upper bound on a segment's length (sizes the scratch of the > 8192-item path);
 * 0 = unknown (n_items is assumed). */
int pg_sort_scores_dev(pg_ctx* ctx, const double* d_scores, const uint32_t* d_seg_offsets,
                       uint32_t n_seg, uint32_t n_items, uint32_t max_segment, int descending,
                       uint32_t* d_out_order);

/* ---- DPP diversity re-rank ------------------------------------------------------------------
 * Replaces DPPSort.KernelMatrix + DPPWithWindow (sort/dpp_sort.go:372-551).  Candidates are rows
 * of `t` (embeddings are L2-normalised in fp64 when normalize_emb != 0), rel = relevance scores
 * (Item.Score).  out_idx receives min(topn, n) indices into the candidate list. */
int pg_dpp(pg_ctx* ctx, const pg_table* t, const uint32_t* cand_rows, const double* rel, uint32_t n,
           double alpha, uint32_t topn, uint32_t window, int normalize_emb, uint32_t* out_idx,
           uint32_t* out_count);

/* The same with every switch of DPPSort.KernelMatrix (sort/dpp_sort.go:372-475):
 *   norm_relevance_score  the dpp_norm_relevance_score experiment parameter (:382-405): 0 none, 1 z-score
 *                         (stat.PopMeanVariance / StdScore), 2 min-max into [1e-6, 1] with max = first, min = last
 *                         candidate.  When the reference bails out ("all item score is zero") the call returns
 *                         PG_ERR_ARITH and the caller keeps the items unchanged, as DPPSort.doSort does.
 *   has_table = 1         embeddings are rows of `t` (DPPSortConfig.TableName set), L2-normalised when normalize_emb;
 *                         hook_emb (optional, [n][hook_dim] fp64: what the functions registered with
 *                         RegisterEmbeddingHook return, :52-58,362) is prepended and the row re-normalised (:419-421);
 *                         always followed by "append 1, scale 1/sqrt 2" (:428-430).
 *   has_table = 0         hook embeddings only (:434-447): normalised when normalize_emb; ensure_pos_similarity
 *                         (DPPSortConfig.EnsurePositiveSim) appends 1 and scales by 1/sqrt 2, otherwise appends 0.
 * out_relevance (optional, [n]) receives the relevance scores as used ("dpp_relevance_score", :410). */
typedef struct {
    double   alpha;
    uint32_t topn, window;
    int      normalize_emb, ensure_pos_similarity, norm_relevance_score, has_table;
    uint32_t hook_dim;
} pg_dpp_options;
int pg_dpp_ex(pg_ctx* ctx, const pg_table* t, const uint32_t* cand_rows, const double* rel, uint32_t n,
              const pg_dpp_options* opt, const double* hook_emb, uint32_t* out_idx, uint32_t* out_count,
              double* out_relevance);

/* ---- SSD diversity re-rank -------------------------------------------------------------------
 * Replaces SSDSort.SSDWithSlidingWindow (sort/ssd_sort.go:346-486) and the embedding treatment of
 * loadEmbeddingCache (:246-252).  Candidates are rows of `t`, given in score-descending order as
 * SSDSort.doSort leaves them (:296); rel = Item.Score.  normalize_emb / ensure_pos_similarity /
 * use_ssd_star / window / gamma are the SSDSortConfig fields of the same names (recconf.go:980-1000);
 * norm_quality_score is the ssd_norm_quality_score experiment parameter (0 none, 1 z-score, 2 min-max).
 * out_idx (capacity n) receives min(topn, n) indices into the candidate list; when the reference would
 * return the items unchanged ("all item score are zeros") it receives 0..n-1 and *out_count = n.
 * out_quality (optional, [n]) receives the normalised quality scores ("ssd_quality_score").
 * PG_ERR_UNSUPPORTED, the context left usable: n > 8192, dim + ensure_pos_similarity > 320, a candidate row outside `t`.
 * SSDSort.Sort / doSort around the window for nq requests on device arrays (the split, the cuts, the gates): pg_ssd_sort_dev. */
int pg_ssd(pg_ctx* ctx, const pg_table* t, const uint32_t* cand_rows, const double* rel, uint32_t n,
           double gamma, uint32_t topn, uint32_t window, int normalize_emb, int ensure_pos_similarity,
           int norm_quality_score, int use_ssd_star, uint32_t* out_idx, uint32_t* out_count,
           double* out_quality);
/* pg_ssd over embeddings the caller holds — emb: [n][dim] fp32 on the host, candidate i's item embedding as loadEmbeddingCache
 * parses it from the item's properties, of any dim with dim + ensure_pos_similarity <= 320 (a table holds 64 / 128 / 192 / 256
 * only).  Everything else as pg_ssd; PG_ERR_UNSUPPORTED for n > 8192 or a wider embedding. */
int pg_ssd_emb(pg_ctx* ctx, const float* emb, uint32_t dim, const double* rel, uint32_t n, double gamma, uint32_t topn,
               uint32_t window, int normalize_emb, int ensure_pos_similarity, int norm_quality_score, int use_ssd_star,
               uint32_t* out_idx, uint32_t* out_count, double* out_quality);

/* ---- item features: typed columns in HBM, assembled by row ----------------------------------
 * Replaces the per-request host boxing of EasyrecAlgoDataGenerator.AddFeatures / GeneratorAlgoData
 * (service/rank/algo_data.go:223-306): one column per feature name (the "context features" of
 * easyrec_predict.proto:150-212), an item that lacks a feature reads the column default
 * (feature.defaultValue, algo_data.go:154-171 — the Go zero value of the column's type).  Columns are
 * keyed by item row; a row index >= rows (UINT32_MAX by convention) means "item without the feature".
 * String features are dictionary-encoded to integer ids by the caller. */
typedef struct pg_features pg_features;
typedef enum { PG_F_I32 = 1, PG_F_I64 = 2, PG_F_F32 = 3, PG_F_F64 = 4 } pg_feature_dtype;
int pg_features_create(pg_ctx* ctx, uint64_t rows, pg_features** out);
int pg_features_destroy(pg_ctx* ctx, pg_features* fs);
/* add or replace column `name`; host_values: [rows] of the dtype, or NULL (every row = default).
 * THE STORED DEFAULT: a column has one default, default_value rounded to the column's dtype — (double)(float)default_value for
 * F32, default_value itself for F64, the integer truncated toward zero for I32 / I64 (-7.9 stores -7).  A NULL fill writes that
 * value into every row and every reader of a row outside the store (gather_i32, gather_f32, pg_features_eval_dev, the FM item
 * records, WhereClause / condition readers) sees that value: a row inside a NULL-filled column and a row outside the store read
 * the same bits.  An I32 / I64 default that is NaN, infinite or outside the dtype's range is PG_ERR_INVALID (the message names
 * the column), refused before anything is allocated or modified: the store stays as it was. */
int pg_features_set_column(pg_ctx* ctx, pg_features* fs, const char* name, int dtype,
                           const void* host_values, double default_value);
int pg_features_column_index(const pg_features* fs, const char* name);   /* -1 if absent */
int pg_features_num_columns(const pg_features* fs);
/* d_out[i][f] = integer column col_idx[f] at d_rows[i] as int32 (int64 saturates) — e.g. the FM field ids */
int pg_features_gather_i32_dev(pg_ctx* ctx, const pg_features* fs, const int32_t* col_idx, uint32_t n_cols,
                               const uint32_t* d_rows, uint32_t n, int32_t* d_out);
/* d_out[i][f] = fmaf((float)value, scale[f], bias[f]) (host arrays [n_cols]; NULL = 1 / 0): dense float
 * inputs with the simplest normalizer fused; richer ones go through pg_expr_*.
 * DIRECT CONVERSION: (float)value rounds ONCE, to nearest-even — an I32 / I64 value converts to fp32 directly, never through a
 * double (an int64 beyond 2^53 would round twice: 2^60 + 2^36 + 1 is 0x5D800001, by way of a double 0x5D800000); an F64 value
 * is (float)double.  Then one fused multiply-add, IEEE throughout: fp32 subnormals are kept (not flushed), an fp64 beyond the
 * fp32 range is +-inf, NaN stays NaN, -0.0 with no scale and no bias is fmaf(-0, 1, +0) = +0.0. */
int pg_features_gather_f32_dev(pg_ctx* ctx, const pg_features* fs, const int32_t* col_idx, uint32_t n_cols,
                               const float* scale, const float* bias, const uint32_t* d_rows, uint32_t n,
                               float* d_out);

/* d_out[i] = the expression with every variable bound to the feature column of that name at d_rows[i] (the column default for a row
 * outside the store), evaluated in fp64 on the device — the numeric `expression` normalizer of a new_feature over item features
 * (service/feature/new_feature_op.go:54-115 with an ExpressionNormalizer, normalizer.go:112-138; service/feature/feature.go:73-78 walks
 * the items one by one) for a candidate batch, without boxing a map per item.  `e`: pg_expr_compile (pairec's default grammar, `${col}`)
 * or pg_expr_compile_typed(…, "antlr") for the arithmetic subset; at most 16 variables, each of which must be a column (PG_ERR_INVALID
 * names the first that is not); PG_ERR_ARITH as pg_expr_eval_dev. */
int pg_features_eval_dev(pg_ctx* ctx, const pg_features* fs, const pg_expr* e, const uint32_t* d_rows, uint32_t n, double* d_out);

/* A Hologres vector recall with its WhereClause (HologresVectorConf.WhereClause, recconf.go:492-497; hologres_vector_recall.go:
 * 23,49-62 and _v2.go:23,56-61: "FROM table WHERE … ORDER BY distance LIMIT n"), in the shape the device serves: `column OP
 * constant` over an int32 / int64 feature column keyed by item row ("create_time > ${time}" with the constant substituted by the
 * caller).  Only rows that pass are candidates; out_count[q] = min(k, rows that pass), the slots behind it carry row UINT64_MAX.
 * metric 0: inner product, descending (pg_recall_topk); 1: squared Euclidean distance, ascending (pg_recall_topk_l2).  Exact.
 * A filter that admits at most an eighth of the table (and at most 8 M rows; knobs "where_compact_max_rows",
 * "where_compact_min_ratio") is served from a compact copy of the admitted rows, gathered per call; a wider one in place, the
 * predicate evaluated where candidates are made.  0.7-6 ms per call of 1-128 queries at 100 M x 128 for any selectivity. */
typedef enum { PG_WHERE_GT = 0, PG_WHERE_GE = 1, PG_WHERE_LT = 2, PG_WHERE_LE = 3, PG_WHERE_EQ = 4, PG_WHERE_NE = 5 } pg_where_op;
int pg_recall_topk_where(pg_ctx* ctx, const pg_table* t, const pg_features* fs, int column, int op, long long value, int metric,
                         const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count);
/* A filtered VIEW of a table: the rows `column OP value` admits, in row order, copied into a table of their own whose recalls answer
 * with the SOURCE's row ids (ties by source row, as pg_recall_topk_where).  For a WhereClause whose constant is fixed when the recall
 * is built (hologres_vector_recall.go:56-61 substitutes "${time}" in the constructor): build the view once per table generation and
 * every recall call — pg_recall_topk[_l2][_dev], pg_coalescer_recall[_l2] / _online_recall of a coalescer created over the view —
 * serves it at the speed of an unfiltered table of that size (its own shadows, statistics and threshold model; requests of many
 * callers share a pass).  A snapshot: later changes of the source or the column do not reach it.  Views serve recall calls only: the
 * recommend calls, and a view as i2i TRIGGER table, are refused (PG_ERR_UNSUPPORTED / PG_ERR_INVALID); rank / DPP / SSD calls take the
 * source table and the recalled ids.  PG_ERR_EMPTY when no row passes (PG_ERR_INVALID is a bad column / operator / feature store).  Destroyed with pg_table_destroy. */
int pg_table_view_create(pg_ctx* ctx, const pg_table* t, const pg_features* fs, int column, int op, long long value, pg_table** out_view);

/* ---- exact IVF-partitioned index ------------------------------------------------------------------
 * The partition index behind the reference's remote vector services (the FAISS service of algorithm/faiss/
 * vectorretrieval.proto:11-20, the Proxima index of HologresVectorRecall(V2), service/recall/hologres_vector_recall.go:23,
 * _v2.go:23), kept EXACT: k-means lists over the table's rows, a rigorous per-(query, list) bound of every score in the list
 * (DESIGN.md 4.1f), and only lists that provably cannot reach the query's K-th score are skipped.
 *   Outputs   bit for bit those of pg_recall_topk[_l2][_dev] on the same table and queries: ids (row_offset + local), order, score
 *             bits, tail padding (UINT64_MAX with -inf / +inf) and out_count.  Limits and error codes are the same too:
 *             1 <= k <= 16384, nq <= 256 (<= 32 when dim > 128); squared Euclidean at dim 64 / 128.
 *   Lifetime  the index references its table and holds no copy of the rows (4 B per row plus n_lists x (dim + 4) x 4 B); the
 *             table must outlive the index.  Read-only after build: recalls from several contexts may run at once, each with
 *             its own context's scratch.
 *   Stale     after pg_table_upload, _fill_* or _swap the table's generation differs from the one the index was built against;
 *             a recall through it is then served by the table's own pass (exact, counted as `stale`) until pg_index_refresh.
 *   Refusals  a view as the source, and tables of >= 2^32 rows, return PG_ERR_UNSUPPORTED.
 *   Fallbacks a table with non-finite values builds, every recall through it is served by the table's pass (`nonfinite`, also
 *             counted for a batch with a non-finite query); a batch of nq queries whose live (row, query) pairs would exceed
 *             index_dense_fraction x rows x nq^0.6 (pg_set_option, default 0.01) goes to the table's pass (`dense`); so does one whose candidate
 *             lists overflow or whose per-call scratch cannot be allocated (`overflow`).  None of these is an error.
 *   Build     PG_ERR_NOMEM when an allocation fails; nothing stays allocated then.
 * params: n_lists 0 = round(4 sqrt(rows)) clamped to [1, 65536] and to rows / 64; train_rows 0 = min(rows, 64 n_lists) (the
 * k-means sample); iters 0 = 8 Lloyd iterations; seed picks the sample and the initial centroids.  NULL = all defaults. */
typedef struct pg_index pg_index;
typedef struct {
    uint32_t n_lists;
    uint32_t train_rows;
    uint32_t iters;
    uint64_t seed;
} pg_index_params;
int pg_index_build(pg_ctx* ctx, const pg_table* t, const pg_index_params* p, pg_index** out);
int pg_index_destroy(pg_ctx* ctx, pg_index* ix);
int pg_index_recall_topk(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                         float* out_scores, uint32_t* out_count);
int pg_index_recall_topk_dev(pg_ctx* ctx, const pg_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                             float* d_out_scores, uint32_t* out_count);
int pg_index_recall_topk_l2(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                            float* out_dist, uint32_t* out_count);
int pg_index_recall_topk_l2_dev(pg_ctx* ctx, const pg_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                                float* d_out_dist, uint32_t* out_count);
typedef struct {
    uint32_t n_lists, dim;
    uint64_t rows, generation;          /* the table's rows and the generation the index was built against */
    float    max_radius, mean_radius;   /* r_L >= max ||x - c_L|| over the rows of list L (mean over non-empty lists) */
    uint32_t largest_list;              /* rows of the largest list */
    uint32_t empty_lists;
    double   build_ms;
    /* recalls through the index: calls, queries, row loads and (row, query) scores of the exact re-scoring (one row load per pair:
     * the scan gathers every pair's row), and the batches served by the table's pass, by reason */
    uint64_t calls, queries, rows_scored, pairs_scored;
    uint64_t fallback_dense, fallback_stale, fallback_nonfinite, fallback_overflow;
    /* rows of the lists live for at least one query of a batch (the union; what a scan loading each live list once would read),
     * summed over the batches scored through the index; the most rows one query's scan (outside its probe) scored in one batch */
    uint64_t rows_live, max_query_scan_rows;
} pg_index_stats_t;
int pg_index_stats(const pg_index* ix, pg_index_stats_t* out);

/* Serving through an index.  pg_index_attach routes every recall of ix's table that runs as a recall job through ix first: the
 * plain calls pg_recall_topk[_l2][_dev], pg_i2i_recall and pg_online_vector_recall, a coalescer's recall / l2 / i2i / online /
 * recommend batches, and pg_recommend_dnn3_dev / _begin / _end.  Not routed: pg_recall_topk_where (filtered), views, the shard
 * group, and pg_index_recall_topk* (whose own fallback is the table's pass).  pg_recall_topk_where goes through the attached index
 * only with the option "index_route_where" set (as pg_index_recall_topk_where, synchronously).  The index's plan is enqueued without a host
 * synchronisation and verified with the job's status words afterwards; when it does not hold — the batch is dense, needs more
 * rounds than "index_plan_rounds" (pg_set_option, default 2), has a non-finite query or overflows its candidate lists — the
 * table's own plans serve the whole batch.  Outputs are bit for bit the table's.  A stale index (the table changed since the
 * build) is skipped.  After a dense or rounds re-plan, batches of that size band (1, 2-8, 9-32, 33-64, 65-256 queries) skip
 * the index for "index_skip_batches" batches (default 64), then try it once more.
 *   attach   at most one index per table (a second replaces the first); PG_ERR_INVALID for a view.  Neither call bumps the
 *            table's generation or drops its statistics; both wait until nothing enqueued reads a replaced index any more.
 *   detach   PG_ERR_INVALID when ix is not attached.  pg_index_destroy refuses an attached index (PG_ERR_INVALID).
 *   stats    plans tried, held and their queries; re-plans by reason; batches that never tried the plan (stale index, or the
 *            size band switched off).  pg_index_stats' calls, queries, pairs, rows_live and fallbacks include the plans. */
int pg_index_attach(pg_ctx* ctx, pg_index* ix);
int pg_index_detach(pg_ctx* ctx, pg_index* ix);
typedef struct {
    uint64_t plans, plans_held, queries_held;
    uint64_t replan_dense, replan_rounds, replan_overflow, replan_nonfinite;
    uint64_t skipped_stale, skipped_switch;   /* batches that never tried the index plan */
} pg_index_serving_stats_t;
int pg_index_serving_stats(const pg_index* ix, pg_index_serving_stats_t* out);
/* Diagnostics of an index's device state (what the search prunes with).
 *   read     copies the build's arrays to host memory: offsets [n_lists + 1] (list L holds perm[offsets[L], offsets[L+1])),
 *            perm [rows] (source rows, ascending within a list), centroids [n_lists][dim], cnorm [n_lists] (>= ||c_L||) and
 *            radius [n_lists] (>= max ||x - c_L|| over the list's rows; 0 for an empty list).  Any output pointer may be NULL.
 *   bounds   U[q][L] for host queries [nq][dim], 1 <= nq <= 256, as the search computes it (the same launch): an upper bound of
 *            every chain score of list L's rows (l2 != 0: of every -d, d the squared Euclidean distance); +inf where a partial
 *            sum could overflow.  out: [nq][n_lists].  Neither needs a current generation.  PG_ERR_INVALID on a NULL ctx or
 *            index (or, for bounds, NULL queries / out or nq out of range). */
int pg_index_read(pg_ctx* ctx, const pg_index* ix, uint32_t* offsets, uint32_t* perm, float* centroids, float* cnorm, float* radius);
int pg_index_bounds(pg_ctx* ctx, const pg_index* ix, const float* queries, uint32_t nq, int l2, float* out);

/* A filtered recall through an index: pg_recall_topk_where (WhereClause `column OP value`) with the index in place of the table
 * (DESIGN.md 4.1h).  Argument checks, error codes and outputs are pg_recall_topk_where's on ix's table, bit for bit: only admitted
 * rows are candidates, out_count[q] = min(k, admitted), padding UINT64_MAX with -inf (metric 1: +inf, distances ascending), no
 * admitted row gives padding and zero counts; at most 32 queries at dim > 128.
 *   Search   the index's search over the filter's lists — each list restricted to the rows the filter admits — the probe
 *            covering min(K, admitted) admitted rows; lists without an admitted row are never probed or scanned.
 *   Lists    built on the device (the predicate as a bitmap in row order, per-list counts, a stable compaction of the index's
 *            permutation) and kept per index, keyed by feature store, column, the column's version (every
 *            pg_features_set_column is a new one), op, value and the index's generation: "index_where_cache" entries (default
 *            4, least recently used evicted; 0 = built per call and freed after it), each admitted x 4 B + (n_lists + 1) x 4 B
 *            of device memory (plus a bitmap of rows / 8 bytes while it is built).  Contexts may share one index.
 *   Fallbacks a stale index, a non-finite table or query, a dense batch (pairs above index_dense_fraction x min(rows, 150 x
 *            admitted) x nq^0.6) and an overflow are answered by pg_recall_topk_where's own search, counted in
 *            pg_index_stats' fallback fields; every call counts in calls, queries, pairs, rows_scored and rows_live.
 * where_read copies a filter's lists (built or from the cache): offsets [n_lists + 1] (list L: perm[offsets[L], offsets[L+1])),
 * perm [admitted] (at most the index's rows), *admitted; any output may be NULL.  where_stats: the cache's builds, hits,
 * evictions, entries held and their device bytes. */
int pg_index_recall_topk_where(pg_ctx* ctx, const pg_index* ix, const pg_features* fs, int column, int op, long long value,
                               int metric, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows,
                               float* out_scores, uint32_t* out_count);
int pg_index_where_read(pg_ctx* ctx, const pg_index* ix, const pg_features* fs, int column, int op, long long value,
                        uint32_t* offsets, uint32_t* perm, uint64_t* admitted);
typedef struct {
    uint64_t builds, hits, evictions;
    uint64_t entries, bytes;            /* the entries the cache holds and their device bytes */
} pg_index_where_stats_t;
int pg_index_where_stats(const pg_index* ix, pg_index_where_stats_t* out);

/* ---- compound WhereClauses ----------------------------------------------------------
 * The clauses deployments write in HologresVectorConf.WhereClause are conjunctions ("status = 1 AND create_time > ${time}",
 * "cat_id IN (3, 7, 12) AND stock > 0"); pg_where serves them everywhere the single `column OP constant` is served.
 *   Grammar   expr  := and ( OR and )*          and := unary ( AND unary )*        unary := NOT unary | '(' expr ')' | term
 *             term  := column OP integer        OP: > >= < <= = == != <>
 *                    | column [NOT] IN '(' integer ( ',' integer )* ')'
 *                    | column [NOT] BETWEEN integer AND integer          (both bounds inclusive, as SQL)
 *             Keywords in any case; columns [A-Za-z_][A-Za-z0-9_]*; integers signed decimal that fit long long (the caller
 *             substitutes "${time}" before compiling).  Columns compare as long long, the logic is two-valued (no NULL).
 *   Limits    16 distinct columns, 64 terms, 1024 IN constants in total (as written), 64 levels of '(' and NOT nesting.
 *   compile   parses only and needs no GPU; column names are kept and resolved against a feature store at each use.  NULL
 *             arguments are PG_ERR_INVALID; everything else that is refused — strings, floats, functions, arithmetic, trailing
 *             text, an integer that overflows, a limit exceeded, hostile nesting — is PG_ERR_PARSE with pg_last_error() naming
 *             the 0-based byte position ("... at position N").
 *   columns   pg_where_num_columns / _column_name: the distinct columns in order of first appearance (NULL out of range).
 *   eval_host evaluates the compiled program on host arrays — cols[i] / dtypes[i] (PG_F_I32 or PG_F_I64) belong to column i
 *             of pg_where_column_name — into out_bits[(rows + 31) / 32]: bit r & 31 of word r >> 5 is set when row r passes,
 *             bits beyond `rows` are zero.  It states what the device kernel reproduces word for word.
 *   Binding   a call that takes a pg_where resolves its columns by name in `fs`: a column the store lacks, one that is not
 *             int32 / int64 or has no values, and a store of fewer rows than the table are PG_ERR_INVALID.  This is the one
 *             error code that differs from the calls the _ex calls extend, which answer a float or value-less column with
 *             PG_ERR_UNSUPPORTED; it holds for a one-comparison clause too (its search, not its binding, is today's path).
 *   Bitmap    a clause of more than one plain comparison is evaluated on the device into a bitmap of rows / 8 bytes (one kernel,
 *             every referenced column read once) that the pg_where keeps: its key is the store, the version of every referenced
 *             column (pg_features_set_column makes a new one), the row count and the device, so a changed column rebuilds it on
 *             the next use.  One bitmap is kept; contexts and threads may share a pg_where (builds are serialised), and a
 *             rebuild never frees a bitmap under a search that still reads it.  A clause that IS one plain comparison
 *             ("stock > 0", also negated or parenthesised) takes pg_recall_topk_where's path unchanged and builds nothing.
 *   _ex calls pg_recall_topk_where_ex, pg_index_recall_topk_where_ex and pg_table_view_create_ex are pg_recall_topk_where,
 *             pg_index_recall_topk_where and pg_table_view_create with the clause in place of (column, op, value): the same
 *             argument checks in the same order, error codes (but for Binding's), padding, out_count, "index_route_where"
 *             routing, fallbacks and counters.  The index keeps a compound clause's filtered lists under the pg_where's identity and its bitmap's epoch
 *             beside the index generation; "index_where_cache" governs eviction as before.
 *   bits      a diagnostic: the device's bitmap for `rows` rows of `fs` (built, or from the cache; a plain comparison too)
 *             into out_bits[(rows + 31) / 32] and the rows it admits; either output may be NULL.  `rows` is the caller's
 *             (at most the store's) and part of the kept bitmap's key: asking for another row count than the table's replaces
 *             the bitmap the recalls use, and their next call rebuilds it.
 *   stats     bitmap builds and cache hits, the last build's device milliseconds, the device bytes held (program + bitmap), the
 *             kept bitmap's epoch and the rows it admits.
 * pg_where_free must not run while a call uses the clause. */
int pg_where_compile(const char* clause, pg_where** out);
int pg_where_free(pg_where* w);
int pg_where_num_columns(const pg_where* w);
const char* pg_where_column_name(const pg_where* w, int i);
int pg_where_eval_host(const pg_where* w, const void* const* cols, const int* dtypes, uint64_t rows, uint32_t* out_bits);
int pg_recall_topk_where_ex(pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, int metric,
                            const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores,
                            uint32_t* out_count);
int pg_index_recall_topk_where_ex(pg_ctx* ctx, const pg_index* ix, const pg_features* fs, const pg_where* w, int metric,
                                  const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores,
                                  uint32_t* out_count);
int pg_table_view_create_ex(pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, pg_table** out_view);
int pg_where_bits(pg_ctx* ctx, const pg_where* w, const pg_features* fs, uint64_t rows, uint32_t* out_bits, uint64_t* out_admitted);
typedef struct {
    uint64_t builds, hits;              /* bitmap builds, and uses that found the kept bitmap current */
    double   last_build_ms;             /* the last build's kernel, device time */
    uint64_t bytes;                     /* device bytes the kept bitmap and its program hold */
    uint64_t epoch, admitted;           /* the kept bitmap's epoch (process-wide, never reused) and the rows it admits */
} pg_where_stats_t;
int pg_where_stats(const pg_where* w, pg_where_stats_t* out);

/* Per-request exclusion lists: the items THIS user has already been shown, taken out inside the vector recall.
 * In the reference that filter is part of the recall: BeVectorRecall.GetItems (service/recall/be_vector_recall.go:63-95) asks its
 * BeFilterNames for query parameters, and berecall.User2ItemExposureFilter.BuildQueryParams (service/recall/berecall/
 * user_item_exposure_filter.go:22-33) puts the user's exposure_list into the vector query, so the engine returns returnCount
 * UNSEEN items.  Deployments without BE run filter/user_item_exposure_filter.go:34-49 (FilterByHistory) behind the recall and
 * are left with fewer than RecallCount candidates for rank.  Here the answer is exact and full: a recall's answer is totally
 * ordered (score, then row), so the first k entries outside a list of n ids lie within the first k + n; one ordinary pass at
 * depth k + (the longest list of the call) holds every request's answer, and one order-preserving compaction on the device cuts
 * it out.
 *   Lists     request q excludes excl_rows[excl_offsets[q] .. excl_offsets[q + 1]): GLOBAL row ids as recalls return them
 *             (row_offset + local row; for a view the source's ids), unsorted, duplicates allowed, at most 4096 per request
 *             (more: PG_ERR_UNSUPPORTED).  An id that cannot occur in the answer — UINT64_MAX, a row outside the table, a row
 *             the clause does not admit — matches nothing.  excl_offsets is host memory [nq + 1] in every call but
 *             pg_exclude_compact_dev; NULL or non-monotone offsets are PG_ERR_INVALID.
 *   compact   pg_exclude_compact_dev is the kernel alone: d_rows / d_scores [nq][k_in] in a recall's output order (they may end
 *             in UINT64_MAX padding), lists and offsets on the device; output slot j of request q is its j-th input entry that
 *             is neither padding nor in its list — relative order and score bits untouched — the slots from the kept count on
 *             carry UINT64_MAX / pad_score, d_out_count[q] (optional) = min(k_out, kept).  1 <= k_out <= k_in <= 16384 and
 *             nq <= 256 (else PG_ERR_UNSUPPORTED / PG_ERR_INVALID); at most 4096 ids per request is a PRECONDITION here (the
 *             offsets are device memory: the caller keeps it; of a longer list the first 4096 ids count).  Outputs must not overlap the inputs.  One launch on the
 *             context's stream, no synchronisation; an empty list costs a copy of the head.  A sharded host (the shard
 *             group, dist.py) has no exclude call of its own: it over-asks its merge by the longest list and calls this after
 *             pg_topk_merge_lists_dev.
 *   recalls   pg_recall_topk_exclude[_dev] return the exact top-k — order, padding (UINT64_MAX with -inf; +inf for metric 1) and
 *             argument checks of the call they extend, in its order: pg_recall_topk[_l2][_dev], or with opts->fs / opts->where
 *             pg_recall_topk_where_ex — over the rows of `t` (the rows the clause admits) that are not in the request's list;
 *             out_count[q] = min(k, candidates - excluded candidates).  opts = NULL is {0, NULL, NULL}; fs without where or
 *             where without fs is PG_ERR_INVALID.  The inner recall runs at k + the longest list through the very search the
 *             plain call uses, so an attached index, "index_route_where", the compact route of a selective clause and views
 *             serve it unchanged and count it as usual; k + the longest list > 16384 is PG_ERR_UNSUPPORTED.  With every list
 *             empty the pass runs at k and the outputs are bit for bit the plain call's.  _dev: queries, lists and outputs
 *             are device memory, offsets and out_count host; both forms return synchronised.
 *   i2i       pg_i2i_recall_exclude is pg_i2i_recall (its checks, in its order) with lists; exclude_trigger != 0 appends each
 *             request's own trigger row to its list — the hole pg_i2i_recall documents — and needs trigger_table == t
 *             (PG_ERR_INVALID otherwise); excl_rows / excl_offsets may then be NULL.  The list with the trigger row holds at
 *             most 4096 ids.
 *   coalescer pg_coalescer_recall_exclude, below. */
typedef struct {
    int metric;                /* 0 inner product (descending), 1 squared Euclidean (ascending) */
    const pg_features* fs;     /* with `where`: candidates restricted to the clause's rows; both NULL = every row */
    const pg_where* where;
} pg_recall_exclude_opts;
int pg_exclude_compact_dev(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t k_in,
                           const uint64_t* d_excl_rows, const uint32_t* d_excl_offsets, uint32_t k_out, float pad_score,
                           uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count);
int pg_recall_topk_exclude(pg_ctx* ctx, const pg_table* t, const float* queries, uint32_t nq, uint32_t k,
                           const uint64_t* excl_rows, const uint32_t* excl_offsets, const pg_recall_exclude_opts* opts,
                           uint64_t* out_rows, float* out_scores, uint32_t* out_count);
int pg_recall_topk_exclude_dev(pg_ctx* ctx, const pg_table* t, const float* d_queries, uint32_t nq, uint32_t k,
                               const uint64_t* d_excl_rows, const uint32_t* excl_offsets, const pg_recall_exclude_opts* opts,
                               uint64_t* d_out_rows, float* d_out_scores, uint32_t* out_count);
int pg_i2i_recall_exclude(pg_ctx* ctx, const pg_table* trigger_table, const uint32_t* trigger_rows, uint32_t n, const pg_table* t,
                          uint32_t k, int exclude_trigger, const uint64_t* excl_rows, const uint32_t* excl_offsets,
                          uint64_t* out_rows, float* out_scores, uint32_t* out_count);

/* ---- ColdStartRecall (csrc/coldstart.hip, csrc/coldstart_host.hpp) ---------------------------------
 * ColdStartRecall.GetCandidateItems runs `SELECT pk FROM t WHERE <WhereClause> ORDER BY <OrderBy | random()> LIMIT n`
 * (module/cold_start_recall_hologres_dao.go:48,76-80,116-153; without a clause every row, cold_start_recall_featurestore_dao.go:
 * 155-169).  pg_cold turns "the rows a clause admits" into a recall answer on the device, in both orders.
 *   create    needs no GPU.  w: the compiled clause, BORROWED (the caller may share it with its vector recalls: one bitmap serves
 *             both) and not to be freed before the pg_cold; NULL = every row of the table.  order_by: NULL, "" or random() in
 *             any case = the random order; otherwise `column`, `column ASC` or `column DESC` (keywords in any case, one column
 *             [A-Za-z_][A-Za-z0-9_]*), the name kept and resolved in `fs` at each use.  Anything else — two columns, an
 *             expression, NULLS FIRST — is PG_ERR_PARSE with the 0-based byte position in pg_last_error() ("... at position N").
 *   Pool      the rows r < rows whose bit is set in the clause's bitmap (pg_where: bit r & 31 of word r >> 5; a one-comparison
 *             clause's bitmap is built too).  sel(j) is the j-th admitted row in ascending row order, 0 <= j < A.
 *   Random    request q with seed[q] (NULL: 0 for every request) gets slot i = row_offset + sel(P(i)), i < min(k, A), where P
 *             is a keyed bijection of [0, A): b = the smallest even integer >= 2 with 2^b >= A, h = b / 2, mask = 2^h - 1; one
 *             application on x < 2^b splits (L, R) = (x >> h, x & mask), runs for r = 0 .. 7
 *                 (L, R) <- (R, L ^ (mix(seed + 0x9E3779B97F4A7C15 * (1 + r * 2^32 + R)) & mask))          (uint64 arithmetic,
 *             mix = the splitmix64 finaliser of pg_mix_sort's draw) and returns (L << h) | R; P(i) applies it to i and again to
 *             the result while that is >= A (cycle walking: a bijection returns to [0, A); 2^b < 4 A, so fewer than four
 *             applications are expected).  Hence: the ids of a request are distinct; with k >= A a request's answer is a
 *             permutation of the pool; and the answer at depth k is a PREFIX of the answer at any larger depth — over-fetching
 *             by the longest exclusion list and pg_exclude_compact_dev give the first k unseen items of the same sequence.
 *             Go's math/rand and Postgres's random() are not reproduced (as with pg_mix_sort's random_position).
 *   Ordered   key of a row = its column value (I32, I64, F32 or F64) as an order-preserving unsigned integer: integers with the
 *             sign bit flipped; floats with -0.0 taken as +0.0 and the usual total-order transform, every NaN greater than every
 *             number and equal to every other NaN (Postgres: first under DESC, last under ASC); F32 orders as its exactly widened
 *             value.  The answer is the admitted rows by (key ascending or descending, then row ascending) cut to min(k, A): ties
 *             break by row.  It is the same for every request of the call, computed once, written nq times; seeds are ignored.
 *   Out       every recall's shape (a pg_fanin_source with score_f64 = 0): out_rows [nq][k] global ids then UINT64_MAX,
 *             out_scores [nq][k] 0.0f (module.NewItem leaves Score zero) then -inf, out_count[q] (optional) = min(k, A).  A = 0
 *             is PG_OK with all padding (the reference returns an empty list).
 *   Limits    1 <= nq <= 256 (else PG_ERR_INVALID), 1 <= k <= 16384 and 1 <= rows < 2^32, no filtered view (PG_ERR_UNSUPPORTED);
 *             fs must cover the table's rows and hold the clause's columns (pg_where's Binding rules) and the order column, numeric
 *             with values (PG_ERR_INVALID); fs may be NULL for a random order without a clause.  Refusals are made on the host,
 *             nothing enqueued, the context left usable.
 *   host      pg_cold_recall_host states the answer on host arrays (bits NULL = every row; order_col / order_dtype the ordered
 *             column's values and PG_F_* type, unused for the random order); the device calls reproduce it bit for bit.
 *   Stream    the pg_cold keeps, per bitmap epoch, the admitted count of every 1 024-row block and its exclusive scan (4 B per
 *             block) beside a reference to the bitmap.  With both current pg_cold_recall_dev only enqueues on the context's stream
 *             and reads nothing back — A comes from the bitmap's build (the `_dev` scratch exception of pg_fanin_merge_dev
 *             applies).  A call that has to build the bitmap or the prefix synchronises the stream, as a pg_where build does; a
 *             call that REPLACES the kept pair first waits for the whole device, so a kernel enqueued earlier never reads freed
 *             memory, and an answer enqueued before a column write is the old columns' answer.  Contexts and threads may share a
 *             pg_cold: builds are serialised.  pg_cold_recall takes host arrays: upload, run, download, synchronise.
 *             pg_cold_free waits for the device; it must not run while a call uses the pg_cold.
 *   stats     prefix builds and uses that found it current, device bytes held (prefix; without a clause the all-rows bitmap
 *             too), the bitmap's epoch (0 without a clause) and the rows it admits. */
typedef struct pg_cold pg_cold;
typedef struct {
    uint64_t prefix_builds, prefix_hits;
    uint64_t bytes;
    uint64_t epoch, admitted;
} pg_cold_stats_t;
int pg_cold_create(const pg_where* w, const char* order_by, pg_cold** out);
int pg_cold_free(pg_cold* c);
int pg_cold_recall_host(const pg_cold* c, const uint32_t* bits, uint64_t rows, uint64_t row_offset, const void* order_col,
                        int order_dtype, const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores,
                        uint32_t* out_count);
int pg_cold_recall_dev(pg_ctx* ctx, const pg_cold* c, const pg_table* t, const pg_features* fs, const uint64_t* d_seed,
                       uint32_t nq, uint32_t k, uint64_t* d_out_rows, float* d_out_scores, uint32_t* d_out_count);
int pg_cold_recall(pg_ctx* ctx, const pg_cold* c, const pg_table* t, const pg_features* fs, const uint64_t* seed, uint32_t nq,
                   uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count);
int pg_cold_stats(const pg_cold* c, pg_cold_stats_t* out);

/* Collaborative-filter recall (U2I2I) over a similarity table resident in HBM (csrc/cf.hip).
 * UserCollaborativeFilterRecall.GetCandidateItems (service/recall/user_collaborative_filter_recall.go:31-80) reads the user's
 * trigger items with their preference scores, expands them into their similar-item lists (swing / etrec) with four goroutines
 * of SELECT ... WHERE item_id IN (...) under a 200 ms timeout (module/user_collaborative_hologres_dao.go:58-216), multiplies
 * every similarity by the trigger's preference (:179-192), sums the products per distinct item in float64
 * (module/user_collaborative_dao.go:38-51), divides by the largest sum unless Normalization is "off" (:61-68), sorts
 * descending and cuts to RecallCount.  ItemCollaborativeFilterRecall (service/recall/item_collaborative_filter_recall.go:40-90)
 * is the one-trigger case with prefer = 1 and normalize = 0.  RealTimeU2IRecall is NOT this call: its DAO keeps the LARGEST
 * sim * prefer term of an item, un-normalised, where this call sums and normalises — pg_rtu2i_* below serves it, trigger
 * weights included.
 *   Table     CSR over the LOCAL rows of an item table `t`: offsets uint64[rows + 1], neighbours uint32[pairs] (local rows of
 *             `t`), similarities float[pairs].  The reference parses similarities from text as float64; here they are stored
 *             fp32, like every table of this engine, and widened exactly when used.  `t` must outlive the similarity table,
 *             must not be a view, and holds at most 2^32 - 1 rows.  A table whose rows were never uploaded has empty lists.
 *   upload    pg_simtable_upload appends the lists of `nrows` consecutive rows from row0; rows arrive in ascending order (row0
 *             at or behind the end of the previous upload; rows skipped keep empty lists); offsets[nrows + 1] are relative to
 *             the call's nbr_rows / sims.  PG_ERR_INVALID, the table left as it was, for a list longer than 1024, a neighbour
 *             >= rows, a non-finite similarity, or a neighbour that appears twice in one list (duplicate-free lists are what
 *             makes the sums deterministic without floating-point atomics).  Synchronous; recalls of other contexts wait.
 *   stale     the table records t's generation at create: after pg_table_swap (or any other write) of `t` a recall returns
 *             PG_ERR_INVALID with a message that names both generations — there is nothing to fall back to.
 *   recall    request q's triggers are trigger_rows / trigger_prefer [trigger_offsets[q] .. trigger_offsets[q + 1]) (local rows
 *             of `t`; at most 256 per request, nq <= 256, 1 <= k <= 16384; else PG_ERR_UNSUPPORTED / PG_ERR_INVALID as the
 *             vector recalls).  The answer is DEFINED, bit for bit:
 *               - triggers j in the order given, within a trigger the list's entries e in stored order;
 *                 term = (double)sim_e * prefer_j (one rounding); the first term of an item IS its score, every later one is
 *                 score = score + term — the order a single goroutine of the reference would take;
 *               - a trigger row of UINT32_MAX or >= rows contributes nothing (an id the reference's SQL does not return); a
 *                 trigger that occurs twice contributes twice; trigger items are not removed from the answer;
 *               - m = the largest score, found with > from 0; with normalize != 0 and m > 0 every score becomes score / m;
 *               - order: score descending, then local row ascending (-0.0 ranks as 0.0); out_rows are global ids (row_offset +
 *                 local row), the first k of that order; slots past the distinct count carry UINT64_MAX and -inf;
 *                 out_count[q] = the valid count; a request without triggers answers 0.
 *             trigger_prefer must be finite: pg_cf_recall checks it (PG_ERR_INVALID), for pg_cf_recall_dev it is a
 *             precondition.  A request whose lists hold more than 65536 pairs in all is never cut: the call returns
 *             PG_ERR_UNSUPPORTED and names the request (the other requests' outputs are written).
 *   opts      NULL = {1, NULL, NULL}.  normalize: the reference's default ("on" unless "off", recconf.go:579).  excl_rows /
 *             excl_offsets: per-request exclusion lists with the meaning, limits and errors they have in
 *             pg_recall_topk_exclude (global ids, at most 4096 per request, k + the longest list <= 16384): the answer is the
 *             first k entries of the same order that are not in the request's list.
 *   _dev      trigger_rows, trigger_prefer, opts->excl_rows and the outputs are device memory; both offset arrays and
 *             out_count (optional) are host memory.  Both forms return synchronised.
 *   Memory    scratch of about 40 B x min(65536, rows) per request of the batch (the global tier's tables and the items to
 *             order: 0.7 GB for 256 requests on a table of >= 65536 rows), kept by the context. */
typedef struct pg_simtable pg_simtable;
typedef struct {
    int normalize;                 /* != 0: divide by the largest score when it is positive */
    const uint64_t* excl_rows;     /* with excl_offsets: per-request exclusion lists; both NULL = none */
    const uint32_t* excl_offsets;  /* host [nq + 1] */
} pg_cf_opts;
int pg_simtable_create(pg_ctx* ctx, const pg_table* t, pg_simtable** out);
int pg_simtable_upload(pg_ctx* ctx, pg_simtable* s, uint64_t row0, uint64_t nrows, const uint64_t* offsets, const uint32_t* nbr_rows,
                       const float* sims);
/* any of the outputs may be NULL; generation = the item table's generation the lists belong to */
int pg_simtable_info(const pg_simtable* s, uint64_t* rows, uint64_t* pairs, uint64_t* rows_uploaded, uint64_t* generation);
int pg_simtable_destroy(pg_ctx* ctx, pg_simtable* s);
int pg_cf_recall(pg_ctx* ctx, const pg_simtable* s, const uint32_t* trigger_rows, const double* trigger_prefer,
                 const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* out_rows, double* out_scores,
                 uint32_t* out_count);
int pg_cf_recall_dev(pg_ctx* ctx, const pg_simtable* s, const uint32_t* d_trigger_rows, const double* d_trigger_prefer,
                     const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* d_out_rows,
                     double* d_out_scores, uint32_t* out_count);

/* RealTimeU2IRecall on the device (csrc/rtu2i.hip, csrc/cf.hip): the user's latest behaviour events become
 * weighted trigger items, the triggers are expanded through a similarity table, the largest term of an item is its score.
 * Reference: service/recall/realtime_u2i_recall.go; RealtimeUser2ItemHologresDao (module/realtime_user2item_hologres_dao.go:
 * 98-343: GetTriggerInfos, ListItemsByUser) over NewRealtimeUser2ItemBaseDao's config (module/realtime_user2item_dao.go:64-136).
 *   compile   pg_rtu2i_compile turns a UserTriggerDaoConf into a pg_rtu2i (host only, no context).
 *             event_names[n_events] is the dictionary that gives events their uint16 codes (code = index).
 *             event_weight / event_play_time ("click:1;buy:3.5") are parsed as the reference does (:96-120): split on ';', then
 *             on ':'; a piece without exactly two parts, or whose number strconv.ParseFloat rejects, is skipped; a later piece
 *             of a name replaces an earlier one; a name outside event_names can never match and is ignored.  A non-empty
 *             event_weight that yields no pair is PG_ERR_INVALID (the reference panics).  A number ParseFloat reads in a form
 *             this front end does not (hexadecimal, '_' between digits) is PG_ERR_UNSUPPORTED.  NULL = "".
 *             weight_expression is the govaluate arithmetic subset of pg_expr_compile_govaluate with the DAO's own function
 *             table (:23-30), which holds ONLY exp: round(...) is refused by name here, as exp is everywhere else; anything
 *             outside the subset (comparators, strings, ...) is PG_ERR_UNSUPPORTED, named in the message.  The only variables
 *             are currentTime and eventTime: any other name is PG_ERR_INVALID, named (in the reference every evaluation would
 *             fail and every weight would be 0); so is an empty expression (no evaluation yields a number: every weight 0).
 *             At most 64 operations, stack depth 8.  exp(x) is Go's pure math.Exp restated operation for operation (the
 *             FreeBSD e_exp.c form; real(cmplx.Exp(complex(x, 0))) = Exp(x) cos(0) = Exp(x)), the same bits on host and device,
 *             within 1 ulp of libm's exp.  Go's amd64 build uses an assembly Exp, so parity with a Go binary is unpinned, like
 *             govaluate's: this restatement is the specification (csrc/expr_prog.hpp go_exp, tests/rtu2i_ref.py).
 *             weight_mode: "sum", "max", or "" / NULL = sum; anything else PG_ERR_INVALID (the reference sums under any name but
 *             "max").  The effective trigger count T = trigger_count ? trigger_count : limit must lie in 1 .. 256, else
 *             PG_ERR_UNSUPPORTED.  pg_rtu2i_trigger_count returns T.
 *   triggers  Request q's events are [event_offsets[q], event_offsets[q + 1]), in the order the reference's SQL returns them
 *             (ORDER BY timestamp DESC, already cut to Limit by the caller): event_rows uint32 (the local row of the item
 *             table with `rows` rows, 1 <= rows < 2^32), event_code uint16, event_play_time double (NULL: all zeros, the
 *             zero value NoUsePlayTimeField leaves), event_time int64; now[q] int64 = currentTime.Unix().  nq <= 256; at
 *             most 1024 events per request: more is PG_ERR_UNSUPPORTED, the request named, the context left usable.
 *             The answer is DEFINED, bit for bit (GetTriggerInfos, :259-330):
 *               - an event whose row is >= rows (UINT32_MAX included) is dropped before anything else;
 *               - an event whose code has a play-time threshold t is dropped when play_time <= t;
 *               - weight = w * e (one rounding): w the event's weight, 1 when its code has none or is >= n_events; e the
 *                 expression over currentTime = (double)now[q], eventTime = (double)event_time;
 *               - events in the order given: the first surviving event of an item sets its weight; a later one does
 *                 weight = weight + w_e (sum), or replaces the weight only when w_e > weight (max);
 *               - an item whose combined weight is not finite is dropped;
 *               - order: weight descending, then the index of the item's first surviving event ascending (-0.0 ranks as 0.0
 *                 and keeps its bits); the first T entries are kept.
 *             out_rows uint32 [nq][T] (padding UINT32_MAX), out_weight double [nq][T] (padding -inf), out_count uint32 [nq].
 *             With Item2ItemTable == "" the reference returns exactly these items, their weights as scores (:104-112).
 *             Deviations, all where the reference's own answer is not defined or not useful: an event of an item the engine
 *             does not hold could take a TriggerCount place in the reference and then match no SQL row; the reference's sort
 *             is undefined with a NaN in it and the expansion needs finite preferences, hence the dropped non-finite weights;
 *             the reference's order of equal weights is map iteration and pdqsort order.
 *             pg_rtu2i_triggers_host is the host statement (no context); pg_rtu2i_triggers takes host arrays;
 *             pg_rtu2i_triggers_dev device arrays (offsets and now stay host memory) and device outputs.  All return
 *             synchronised.
 *   expand    pg_rtu2i_expand[_dev]: arguments, limits and errors of pg_cf_recall[_dev]; opts->normalize is ignored, the
 *             exclusion lists mean what they mean there.  DEFINED answer: triggers in the order given, entries in stored order,
 *             term = (double)sim * prefer (one rounding); the first term of an item is its score, a later one replaces it only
 *             when term > score — ListItemsByUser's descending sort followed by uniqItems (:203-204), the ±0.0 case decided
 *             by order; no division by the largest score; order, cut, padding, counts, tiers and the 65536-pair report as
 *             in pg_cf_recall.
 *   recall    pg_rtu2i_recall[_dev]: events in, out_rows uint64 [nq][k] and out_scores double [nq][k] out (the shape
 *             pg_fanin_merge_dev takes with score_f64 != 0), out_count optional.  Equal to pg_rtu2i_triggers followed by
 *             pg_rtu2i_expand over `s` (rows = the rows of its item table), byte for byte; the trigger lists stay in device
 *             memory and the two kernels follow each other on the stream with no host read-back between them.  _dev: events,
 *             opts->excl_rows and outputs are device memory; offsets, now and out_count host memory.  Returns synchronised.
 *   Not served (refused or out of scope): DiversityRules / PropertyFields (DiversityTriggers), the BE and FeatureStore DAOs,
 *             MergeMode "snake", the recall's cache line.  The U2I2X2I DAO is pg_rtu2i_x_recall below. */
typedef struct pg_rtu2i pg_rtu2i;
typedef struct {
    const char* weight_expression;
    const char* event_weight;
    const char* event_play_time;
    const char* const* event_names;
    uint32_t n_events;
    const char* weight_mode;
    uint32_t trigger_count;
    uint32_t limit;
} pg_rtu2i_conf;
int pg_rtu2i_compile(const pg_rtu2i_conf* conf, pg_rtu2i** out);
int pg_rtu2i_free(pg_rtu2i* c);
int pg_rtu2i_trigger_count(const pg_rtu2i* c);
int pg_rtu2i_triggers_host(const pg_rtu2i* c, uint64_t rows, const uint32_t* event_rows, const uint16_t* event_code,
                           const double* event_play_time, const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now,
                           uint32_t nq, uint32_t* out_rows, double* out_weight, uint32_t* out_count);
int pg_rtu2i_triggers(pg_ctx* ctx, pg_rtu2i* c, uint64_t rows, const uint32_t* event_rows, const uint16_t* event_code,
                      const double* event_play_time, const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now,
                      uint32_t nq, uint32_t* out_rows, double* out_weight, uint32_t* out_count);
int pg_rtu2i_triggers_dev(pg_ctx* ctx, pg_rtu2i* c, uint64_t rows, const uint32_t* d_event_rows, const uint16_t* d_event_code,
                          const double* d_event_play_time, const int64_t* d_event_time, const uint32_t* event_offsets,
                          const int64_t* now, uint32_t nq, uint32_t* d_out_rows, double* d_out_weight, uint32_t* d_out_count);
int pg_rtu2i_expand(pg_ctx* ctx, const pg_simtable* s, const uint32_t* trigger_rows, const double* trigger_prefer,
                    const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* out_rows,
                    double* out_scores, uint32_t* out_count);
int pg_rtu2i_expand_dev(pg_ctx* ctx, const pg_simtable* s, const uint32_t* d_trigger_rows, const double* d_trigger_prefer,
                        const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* d_out_rows,
                        double* d_out_scores, uint32_t* out_count);
int pg_rtu2i_recall(pg_ctx* ctx, pg_rtu2i* c, const pg_simtable* s, const uint32_t* event_rows, const uint16_t* event_code,
                    const double* event_play_time, const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now,
                    uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count);
int pg_rtu2i_recall_dev(pg_ctx* ctx, pg_rtu2i* c, const pg_simtable* s, const uint32_t* d_event_rows, const uint16_t* d_event_code,
                        const double* d_event_play_time, const int64_t* d_event_time, const uint32_t* event_offsets,
                        const int64_t* now, uint32_t nq, uint32_t k, const pg_cf_opts* opts, uint64_t* d_out_rows,
                        double* d_out_scores, uint32_t* out_count);

/* U2I2X2I recall over an X table resident in HBM (csrc/x2i.hip, csrc/x2i_host.hpp): trigger items -> their X
 * values (category, author, tag list) -> the items listed under each X.  UserCollaborativeFilterRecall and RealTimeU2IRecall
 * switch to this two-hop form as soon as a config names Item2XTable and X2ItemTable (NewUserCollaborativeDao,
 * module/user_collaborative_dao.go:24-26).  Both DAOs (module/user_collaborative_u2i2x2i_hologres_dao.go:73-348,
 * module/realtime_user2item_u2i2x2i_hologres_dao.go:94-270) split every trigger item's xKey on XDelimiter and add the trigger's
 * preference to each X (xPreferScoreMap[x] += prefer, :196-211 / :161-175), walk the X2ItemTable row "id:score,id:score,..." of
 * every distinct X, skip the ids that are trigger items (:311-315 / :242-246) and give every other entry the score xPrefer[x],
 * times the entry's score if it has one.  The collaborative DAO sums the entries of an item in float64 and divides by the
 * largest sum unless Normalization is "off" (mergeUserCollaborativeItemsResult, user_collaborative_dao.go:38-68); the realtime
 * DAO sorts descending and keeps an item's first, largest entry (uniqItems, :262-263) and normalises nothing.  The order of the
 * reference's float64 additions depends on goroutines and map iteration, and it has no test or golden vector for either DAO:
 * the definition below fixes one order, and parity is against this restatement (reference parity unpinned, as for top-K).
 *   Table     two CSR structures over the LOCAL rows of an item table `t` and n_x X values, which the caller numbers
 *             0 .. n_x - 1 (its dictionary, as it numbers items by row): item -> X: offsets uint64[rows + 1], x_ids uint32[];
 *             X -> items: offsets uint64[n_x + 1], item_rows uint32[] (local rows of `t`), scores float[].  Scores are stored
 *             fp32 and widened exactly when used; an entry without a score in the reference is stored as 1.0 (prefer * 1.0 has
 *             prefer's bits).  1 <= n_x < 2^32 - 1; `t` must outlive the X table, must not be a view and holds fewer than
 *             2^32 - 1 rows.  Keys never uploaded have empty lists.
 *   upload    pg_xtable_upload_item2x appends the X lists of `nrows` consecutive rows from row0, pg_xtable_upload_x2item the
 *             item lists of `nx` consecutive X from x0; each side ascending and append-only (the first key at or behind the end
 *             of the side's previous upload; keys skipped keep empty lists); offsets[n + 1] index the call's own arrays.
 *             PG_ERR_INVALID, the table left as it was, for offsets that descend, an item's X list longer than 64, an X's item
 *             list longer than 1024, an x id >= n_x, an item row >= rows, a non-finite score, or an id twice in one list
 *             (duplicate-free lists are what makes the sums deterministic without floating-point atomics; the reference's "a
 *             category appears several times" is across items, and that is served).  Synchronous; recalls of other contexts
 *             wait.  Lock order: the context, the item table, then the X table.
 *   stale     the table records t's generation at create: after pg_table_swap (or any other write) of `t` a recall returns
 *             PG_ERR_INVALID with a message that names both generations.
 *   recall    request q's triggers are trigger_rows / trigger_prefer [trigger_offsets[q] .. trigger_offsets[q + 1]) (local rows
 *             of `t`; at most 256 per request — the collaborative DAO's shuffle cut of more than 200 triggers is the
 *             caller's — nq <= 256, 1 <= k <= 16384; errors as pg_cf_recall).  The answer is DEFINED, bit for bit:
 *               - hop 1: triggers in the order given, within a trigger its X list in stored order; the first trigger that
 *                 names an X sets xPrefer[x] = prefer, every later one does xPrefer[x] = xPrefer[x] + prefer; a trigger row of
 *                 UINT32_MAX or >= rows contributes nothing; a trigger that occurs twice contributes twice (a deviation from the
 *                 SQL IN, which returns a row once: the caller's trigger map makes triggers distinct); the request's distinct
 *                 X stand in order of first appearance; an X whose summed preference is not finite is dropped before hop 2
 *                 (the reference's sort is undefined with NaN or Inf in it: pg_rtu2i_triggers' rule);
 *               - hop 2: the X in that order, within an X its item list in stored order; an item that is ANY of the request's
 *                 trigger rows is skipped — it takes no part in the sums and never counts towards the maximum;
 *                 term = xPrefer[x] * (double)score (one rounding); sum rule: the first term of an item is its score, every
 *                 later one does score = score + term; max rule: a later term replaces the score only when term > score;
 *               - sum rule only: m = the largest score, found with > from 0; with normalize != 0 and m > 0 every score
 *                 becomes score / m;
 *               - order: score descending, then local row ascending (-0.0 ranks as 0.0 and keeps its bits); out_rows are
 *                 global ids, the first k of that order; padding UINT64_MAX / -inf; out_count[q] = the valid count; a request
 *                 with no triggers, no X, or nothing but trigger items answers 0.
 *             Never cut silently: a request that reaches more than 1024 distinct X (counted before the non-finite ones are
 *             dropped), or whose X lists (those of the X kept for hop 2, skipped trigger items included) hold more than 65536
 *             (X, item) pairs in all, makes the call return PG_ERR_UNSUPPORTED; the message names the smallest such request and
 *             the limit it broke (the X limit is tested first); that request answers 0, the other requests' outputs and
 *             counts are written, the context stays usable.  trigger_prefer must be finite: the host-array forms check it
 *             (PG_ERR_INVALID), for pg_x2i_recall_dev it is a precondition.
 *   opts      NULL = {1, 0, NULL, NULL}.  normalize as in pg_cf_opts; max_rule != 0: the realtime DAO's reduction, normalize
 *             ignored; excl_rows / excl_offsets: per-request exclusion lists with the meaning, limits and errors they have in
 *             pg_cf_recall (global ids, at most 4096 per request, k + the longest list <= 16384).
 *   tiers     a request of at most min("cf_lds_max_pairs", 5120) pairs keeps its item table in LDS — this kernel's table has
 *             10240 slots, 2048 fewer than pg_cf_recall's, because the staged X (up to 1024) live in LDS beside it; above, in
 *             the request's slice of context scratch.  Both tiers give the same bits.
 *   _dev      trigger_rows, trigger_prefer, opts->excl_rows and the outputs are device memory; both offset arrays and
 *             out_count (optional) are host memory.  Both forms return synchronised.
 *   _host     pg_x2i_recall_host is the host statement over host CSR arrays (no context, no HIP): the same arguments, limits,
 *             errors and bits; the CSR is held to what the uploads accept (PG_ERR_INVALID otherwise).
 *   rtu2i     pg_rtu2i_x_recall[_dev]: the events of pg_rtu2i_recall[_dev], a pg_xtable in place of the pg_simtable; max_rule is
 *             forced on.  Equal to pg_rtu2i_triggers (rows = the rows of the item table) followed by pg_x2i_recall with
 *             max_rule = 1, byte for byte; the trigger lists stay in device memory and the two kernels follow each other on
 *             the stream with no host read-back between them.
 *   Memory    scratch of about 40 B x min(65536, rows) per request of the batch (the global tier's tables and the items to
 *             order: 0.7 GB for 256 requests on a table of >= 65536 rows), in a slot of its own, kept by the context.
 *   Not served: the shuffle cut of more than 200 triggers, string X values and ids (the caller holds the dictionaries),
 *             "null" or empty ids in an X row, the BE and FeatureStore DAOs. */
typedef struct pg_xtable pg_xtable;
typedef struct {
    int normalize;                 /* != 0: divide by the largest score when it is positive (sum rule only) */
    int max_rule;                  /* != 0: an item keeps its largest term; normalize is ignored */
    const uint64_t* excl_rows;     /* with excl_offsets: per-request exclusion lists; both NULL = none */
    const uint32_t* excl_offsets;  /* host [nq + 1] */
} pg_x2i_opts;
int pg_xtable_create(pg_ctx* ctx, const pg_table* t, uint32_t n_x, pg_xtable** out);
int pg_xtable_upload_item2x(pg_ctx* ctx, pg_xtable* s, uint64_t row0, uint64_t nrows, const uint64_t* offsets, const uint32_t* x_ids);
int pg_xtable_upload_x2item(pg_ctx* ctx, pg_xtable* s, uint32_t x0, uint32_t nx, const uint64_t* offsets, const uint32_t* item_rows,
                            const float* scores);
/* any of the outputs may be NULL; generation = the item table's generation the lists belong to */
int pg_xtable_info(const pg_xtable* s, uint64_t* rows, uint32_t* n_x, uint64_t* i2x_pairs, uint64_t* x2i_pairs, uint64_t* generation);
int pg_xtable_destroy(pg_ctx* ctx, pg_xtable* s);
int pg_x2i_recall(pg_ctx* ctx, const pg_xtable* s, const uint32_t* trigger_rows, const double* trigger_prefer,
                  const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* out_rows,
                  double* out_scores, uint32_t* out_count);
int pg_x2i_recall_dev(pg_ctx* ctx, const pg_xtable* s, const uint32_t* d_trigger_rows, const double* d_trigger_prefer,
                      const uint32_t* trigger_offsets, uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* d_out_rows,
                      double* d_out_scores, uint32_t* out_count);
int pg_x2i_recall_host(uint64_t rows, uint64_t row_offset, uint32_t n_x, const uint64_t* i2x_off, const uint32_t* i2x_ids,
                       const uint64_t* x2i_off, const uint32_t* x2i_rows, const float* x2i_scores, const uint32_t* trigger_rows,
                       const double* trigger_prefer, const uint32_t* trigger_offsets, uint32_t nq, uint32_t k,
                       const pg_x2i_opts* opts, uint64_t* out_rows, double* out_scores, uint32_t* out_count);
int pg_rtu2i_x_recall(pg_ctx* ctx, pg_rtu2i* c, const pg_xtable* s, const uint32_t* event_rows, const uint16_t* event_code,
                      const double* event_play_time, const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now,
                      uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* out_rows, double* out_scores,
                      uint32_t* out_count);
int pg_rtu2i_x_recall_dev(pg_ctx* ctx, pg_rtu2i* c, const pg_xtable* s, const uint32_t* d_event_rows, const uint16_t* d_event_code,
                          const double* d_event_play_time, const int64_t* d_event_time, const uint32_t* event_offsets,
                          const int64_t* now, uint32_t nq, uint32_t k, const pg_x2i_opts* opts, uint64_t* d_out_rows,
                          double* d_out_scores, uint32_t* out_count);

/* List recall over a hot table resident in HBM (csrc/hot.hip, csrc/hot_host.hpp): UserGroupHotRecall,
 * UserGlobalHotRecall and UserTopicRecall as one primitive with three modes.  UserGroupHotRecall
 * (module/user_group_hot_recall_hologres_dao.go:47-140) expands the user's trigger id into one or several trigger_ids, reads each
 * one's item_ids row — entries "id", "id:source" or "id:source:score" —, concatenates them, sorts by score descending and cuts to
 * RecallCount.  UserGlobalHotRecall (module/user_global_hot_recall_hologres_dao.go:50-149) reads one list of the same entries,
 * gives an entry without a score rand.Float64(), and sorts and cuts only a list longer than RecallCount (:144-148).
 * UserTopicRecall (module/user_topic_mysql_dao.go:58-138) gives each of the user's topics int(value / total * RecallCount)
 * places and concatenates the heads of the topics' article lists in stored order.  The reference's sort.Sort is unstable and
 * its draws are Go's math/rand stream: the definition below fixes the ties and the draws, and parity is against this
 * restatement (reference parity unpinned, as for top-K).
 *   Table     a CSR over n_triggers trigger indices, which the caller numbers 0 .. n_triggers - 1 (its dictionary of trigger_id /
 *             topic strings, as it numbers items by row) and the LOCAL rows of an item table `t`: offsets uint64[n_triggers + 1],
 *             item_rows uint32[], scores double[] (utils.ToFloat yields float64, and hot scores are counts that fp32 would merge
 *             into ties), source uint8[]: bits 0-6 = an index into the caller's RetrieveId dictionary, 0 = the recall's own name
 *             (the one-part form, or an empty second part); PG_HOT_UNSCORED (bit 7) set = the entry carries no score (the one-
 *             and two-part forms).  1 <= n_triggers < 2^32 - 1; `t` must outlive the hot table and must not be a view.  Triggers
 *             never uploaded have empty lists.
 *   upload    pg_hottable_upload appends the lists of `ntrig` consecutive triggers from trig0, ascending and append-only (trig0 at
 *             or behind the end of the previous upload; triggers skipped keep empty lists); offsets[ntrig + 1] index the call's
 *             own arrays.  PG_ERR_INVALID, the table left as it was, for offsets that descend, a list longer than
 *             PG_HOT_MAX_ENTRIES, an item row >= rows, a non-finite score, a source of 0xFF (the output padding), an entry marked
 *             unscored whose score is not 0, or a table of 2^40 entries.  A row twice in a list is allowed: the reference keeps
 *             duplicates and nothing here accumulates.  Synchronous: it waits for everything enqueued on the device first.  Lock
 *             order: the context, the item table, then the hot table.
 *   stale     the table records t's generation at create: after pg_table_swap (or any other write) of `t` a recall returns
 *             PG_ERR_INVALID with a message that names both generations.
 *   recall    request q's triggers are triggers [trigger_offsets[q] .. trigger_offsets[q + 1]) (trigger_value beside them, read
 *             in PG_HOT_TOPIC only, else it may be NULL).  The answer is DEFINED, bit for bit:
 *               - concatenation: the request's triggers in the order given, within a trigger its entries in stored order;
 *                 position p counts from 0 over it, n is its length.  A trigger of UINT32_MAX or >= n_triggers contributes
 *                 nothing (a trigger_id without a row); a trigger given twice contributes twice.
 *               - scores: a scored entry has its stored score, bits preserved (-0.0, subnormals).  An unscored entry has 0.0 in
 *                 PG_HOT_GROUP and PG_HOT_TOPIC (module.NewItem), and in PG_HOT_GLOBAL the draw
 *                 u(q, p) = (double)(x >> 11) * 2^-53, x = the splitmix64 finaliser — x ^= x >> 30, x *= 0xBF58476D1CE4E5B9,
 *                 x ^= x >> 27, x *= 0x94D049BB133111EB, x ^= x >> 31, as pg_mix_sort's draw — of
 *                 seed[q] + 0x9E3779B97F4A7C15 * (1 + p) in uint64 arithmetic (seed NULL = 0).
 *               - order: score descending, then p ascending; -0.0 ranks as 0.0.
 *               - PG_HOT_GROUP: always ordered, then cut to min(k, n).
 *               - PG_HOT_GLOBAL: with n <= k the concatenation as stored, draws included, not sorted; with n > k the order
 *                 above, cut to k.
 *               - PG_HOT_TOPIC: never sorted.  v_j = trigger_value[j], 0 taken as 0.5 (:75-77); total = their sequential fp64
 *                 sum in trigger order over ALL the request's triggers, absent ones included (the reference counts a topic it
 *                 later finds no articles for); take_j = (int64)((v_j / total) * (double)k) — two roundings, truncation;
 *                 trigger j contributes its first min(take_j, len_j) entries; the concatenation is cut to k.  The random pick
 *                 of TopicNum topics (:94-100) is the caller's.
 *               - out_rows [nq][k]: row_offset + local row, then UINT64_MAX; out_scores [nq][k]: fp64, then -inf; out_source
 *                 [nq][k]: bits 0-6 of the entry's source, then PG_HOT_PAD_SOURCE; out_count[q] = min(k, n) (TOPIC: of the cut
 *                 concatenation).  Rows and scores are a pg_fanin_source with score_f64 = 1.
 *   Limits    1 <= nq <= 256 and a known mode (else PG_ERR_INVALID); at most 256 triggers per request and 1 <= k <= 16384
 *             (PG_ERR_UNSUPPORTED); n <= PG_HOT_MAX_ENTRIES per request: beyond it the call is refused with PG_ERR_UNSUPPORTED
 *             naming the smallest such request.  PG_HOT_TOPIC: every value finite and >= 0, else PG_ERR_INVALID naming request
 *             and trigger.  Every refusal is made on the host — the table keeps a host copy of its offsets — with nothing
 *             enqueued and the context left usable.
 *   _dev      triggers, trigger_value and trigger_offsets are HOST memory (user features, at most 256 per request; staged with
 *             one copy on the context's stream); d_seed (NULL = 0) and the outputs are device memory, d_out_source and
 *             d_out_count optional.  Enqueue-only on the context's stream, one launch, no synchronisation (the scratch-growth
 *             exception of pg_fanin_merge_dev applies).
 *   pg_hot_recall  host arrays throughout (seed [nq] or NULL): upload, run, download, synchronise.
 *   _host     pg_hot_recall_host is the host statement over host CSR arrays (no context, no HIP): the same arguments, limits,
 *             errors and bits; the CSR is held to what the upload accepts (PG_ERR_INVALID otherwise).
 *   Kernel    one workgroup of 1024 lanes per request; a request of at most 8192 padded entries orders its 16-byte records
 *             in LDS, a longer one in its slice of context scratch (16 B x the padded count); TOPIC, and GLOBAL with n <= k,
 *             write straight from the gather.  Both tiers give the same bits.
 *   Not here  exclusion lists (the reference filters after the recall: pg_bloom_filter_dev and the count filters take the
 *             answer); the per-entry source through pg_fanin_merge_dev (the fan-in attributes a list to one source; the plane
 *             is the caller's); the feature-store, tablestore and Redis DAO variants' text formats; ContextItemRecall. */
#define PG_HOT_GROUP 0
#define PG_HOT_GLOBAL 1
#define PG_HOT_TOPIC 2
#define PG_HOT_MAX_ENTRIES 65536u
#define PG_HOT_UNSCORED 0x80u
#define PG_HOT_PAD_SOURCE 0xFFu
typedef struct pg_hottable pg_hottable;
int pg_hottable_create(pg_ctx* ctx, const pg_table* t, uint32_t n_triggers, pg_hottable** out);
int pg_hottable_upload(pg_ctx* ctx, pg_hottable* h, uint32_t trig0, uint32_t ntrig, const uint64_t* offsets, const uint32_t* item_rows,
                       const double* scores, const uint8_t* source);
/* any of the outputs may be NULL; generation = the item table's generation the lists belong to */
int pg_hottable_info(const pg_hottable* h, uint64_t* rows, uint32_t* n_triggers, uint64_t* pairs, uint32_t* triggers_uploaded,
                     uint64_t* generation);
int pg_hottable_destroy(pg_ctx* ctx, pg_hottable* h);
int pg_hot_recall_dev(pg_ctx* ctx, const pg_hottable* h, int mode, const uint32_t* triggers, const double* trigger_value,
                      const uint32_t* trigger_offsets, const uint64_t* d_seed, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                      double* d_out_scores, uint8_t* d_out_source, uint32_t* d_out_count);
int pg_hot_recall(pg_ctx* ctx, const pg_hottable* h, int mode, const uint32_t* triggers, const double* trigger_value,
                  const uint32_t* trigger_offsets, const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows,
                  double* out_scores, uint8_t* out_source, uint32_t* out_count);
int pg_hot_recall_host(uint64_t rows, uint64_t row_offset, uint32_t n_triggers, const uint64_t* offsets, const uint32_t* item_rows,
                       const double* scores, const uint8_t* source, int mode, const uint32_t* triggers, const double* trigger_value,
                       const uint32_t* trigger_offsets, const uint64_t* seed, uint32_t nq, uint32_t k, uint64_t* out_rows,
                       double* out_scores, uint8_t* out_source, uint32_t* out_count);

/* Fan-in + UniqueFilter on the device (csrc/fanin.hip): the answers of a request's recalls merged into one
 * candidate list without leaving device memory.  RecallService.GetItems (service/recall.go:53-153; the fan-in :126-150) runs
 * every recall of the scene's category and concatenates what they return; UniqueFilter (filter/unique_filter.go:26-49) dedups
 * by item id: the first occurrence wins, a later one only leaves its score in RecallScores[its RetrieveId].
 *   Sources   1 .. PG_FANIN_MAX_SOURCES per call, nq <= 256 requests.  Source s: d_rows uint64 [nq][k] — global row ids of ONE
 *             item table (every id of the call belongs to it), UINT64_MAX = padding, anywhere in a list — and d_scores [nq][k],
 *             float (score_f64 = 0: the vector recalls, pg_i2i_recall) or double (score_f64 != 0: pg_cf_recall_dev).  1 <= k and
 *             cap = the sum of the sources' k <= PG_FANIN_MAX_CAP (pg_recommend_dnn3_dev's limit for k); anything else is
 *             PG_ERR_UNSUPPORTED / PG_ERR_INVALID as in pg_exclude_compact_dev, the context left usable.  The k are host values,
 *             every pointer is device memory; outputs must not overlap inputs.
 *   Answer    DEFINED bit for bit: UniqueFilter over the concatenation "sources as given, entries in list order, padding
 *             dropped" (the reference's source order is goroutine completion order; here it is the order given).  No score is
 *             touched by arithmetic: doubles travel as bits (NaN payloads, -0.0, infinities, subnormals survive), floats are
 *             widened exactly as vector_recall.go:98 does (a signalling NaN comes out quiet, as from any conversion).
 *               d_out_rows [nq][cap]            the distinct ids in order of first occurrence, then UINT64_MAX
 *               d_out_score [nq][cap] fp64      the FIRST occurrence's score (Item.Score); padding -inf
 *               d_out_source [nq][cap] uint8    the first occurrence's source (RetrieveId); padding 0xFF
 *               d_out_recall_scores [n_sources][nq][cap] fp64 (optional)
 *                                               per slot and source that source's score for the item
 *                                               (RecallScores[RetrieveId]); where a source holds the id more than once, its LAST
 *                                               occurrence's (unique_filter.go:43 overwrites) — Item.Score stays the first's;
 *                                               where it does not hold the item, and in padding slots, the quiet NaN
 *                                               0x7FF8000000000000
 *               d_out_source_mask [nq][cap] uint32 (optional)
 *                                               bit s set iff source s holds the item; padding 0.  The reference creates
 *                                               RecallScores only once a duplicate is seen: a mask with more than one bit is
 *                                               that condition for duplicates across recalls (for an id repeated inside one
 *                                               recall only, the reference also creates the map, with that recall's last
 *                                               score alone — which is what the plane carries either way)
 *               d_out_count [nq]                the number of distinct ids
 *             AlgoScores are not merged: recalls carry none.
 *   Tiers     one workgroup per request and an open-addressed table keyed by id; the walk takes PG_FANIN_CHUNK positions at a
 *             time.  cap <= PG_FANIN_LDS_MAX_CAP ("fanin_lds_max_cap") and ids that span less than 2^32 - 1 keep the table in
 *             LDS, keyed on the 32-bit distance to the request's smallest id; everything else — a larger cap, ids further apart
 *             — uses context scratch with full 64-bit keys (12 B x the power of two >= 2 cap, per request).  Two ids that differ
 *             only above bit 32 are never merged.
 *   Stream    one launch on the context's stream, no synchronisation (pg_synchronize, or any later call that does).  One
 *             exception, which holds for every `_dev` stage below that says "no synchronisation": a call whose scratch layout
 *             no longer fits its slot of the context's arena waits for the stream before the slot is freed and reallocated
 *             (kernels enqueued earlier hold the old address).  Slots grow in whole MiB and never shrink, so a serving loop
 *             meets this while its shapes still grow, not in steady state ("Stream order is the only fence"). */
#define PG_FANIN_MAX_SOURCES 8
#define PG_FANIN_MAX_CAP 16384
#define PG_FANIN_LDS_MAX_CAP 8192
#define PG_FANIN_CHUNK 1024
typedef struct {
    const uint64_t* d_rows;    /* [nq][k] */
    const void*     d_scores;  /* [nq][k] float, or double with score_f64 != 0 */
    uint32_t        k;
    int             score_f64;
} pg_fanin_source;
int pg_fanin_merge_dev(pg_ctx* ctx, const pg_fanin_source* sources, uint32_t n_sources, uint32_t nq, uint64_t* d_out_rows,
                       double* d_out_score, uint8_t* d_out_source, double* d_out_recall_scores, uint32_t* d_out_source_mask,
                       uint32_t* d_out_count);

/* Recall quotas and the coarse-rank cut on the device (csrc/trim.hip): the merged candidates of a request cut
 * down between UniqueFilter and RankService.Rank (service/user_recommend.go:105-137) without leaving device memory.
 * PriorityAdjustCountFilter (filter/priority_adjust_count_filter.go:80-251, recconf.AdjustCountConfig) sorts the union by
 * Item.Score, groups it by RetrieveId and keeps a quota per recall in the order the config names them; GeneralRank's actions
 * (service/general_rank/action.go:61-83) sort by the coarse score and keep the first RetainNum (AdjustCountFilter with
 * ShuffleItem false, filter/adjust_count_filter.go:58-71).  Both are: order by a score, keep the first n_c entries of each class
 * of sources, class after class.
 *   In        pg_fanin_merge_dev's outputs as they are, nq <= 256 requests of cap <= PG_TRIM_MAX_CAP entries: d_rows [nq][cap]
 *             uint64, d_score [nq][cap] fp64, d_source [nq][cap] uint8 (optional when the single rule is PG_TRIM_ANY), d_count
 *             [nq] (optional), and what is carried along: d_planes_f64 [n_f64][nq][cap] (optional: the per-recall scores),
 *             d_source_mask [nq][cap] (optional), d_planes_f32 [n_f32][nq][cap] (optional: algorithm scores); at most
 *             PG_TRIM_MAX_PLANES planes each.  An entry is padding if its row is UINT64_MAX or its position is >= d_count[q];
 *             padding may sit anywhere, is dropped and never counted.
 *   Rules     host values, 1 .. PG_TRIM_MAX_RULES of {source, type, count}: type PG_TRIM_FIX or PG_TRIM_ACCUMULATE
 *             (AdjustCountConfig.Type "fix" / "accumulator"), source < PG_TRIM_MAX_SOURCES, or PG_TRIM_ANY = every source,
 *             valid only as the single rule (the AdjustCountFilter / top-N case).
 *   Answer    DEFINED bit for bit — priority_adjust_count_filter.go:92-203 with ensureDiversity == false:
 *               1. a request's real entries are ordered by d_score descending exactly as pg_sort_scores_dev orders them:
 *                  -0.0 equals +0.0, NaN sorts last, ties keep input position.  (The reference shuffles the first half of the
 *                  list and sorts unstably, :88-92, which only randomises the order among equal scores; here it is fixed.)
 *               2. they are grouped by source in that order (:103-104); entries whose source no rule names are dropped;
 *               3. rules apply in the order given (:143-203): FIX takes the first min(len, count) entries of its source and
 *                  leaves the accumulator alone (:145-150); ACCUMULATE takes the first min(len, count - acc) and adds what it
 *                  took to acc (:193-200);
 *               4. the output is the takes concatenated in rule order, then padding: row UINT64_MAX, score -inf, source 0xFF,
 *                  fp64 planes the quiet NaN 0x7FF8000000000000, mask 0, fp32 planes 0; d_out_count[q] = the number taken.
 *             Every carried array is gathered through the same permutation; no value meets arithmetic, doubles and floats
 *             travel as bits.  Outputs are [nq][out_cap] (planes [n][nq][out_cap]) with out_cap from pg_trim_out_cap; an output
 *             is required exactly where its input is given; outputs must not overlap inputs.
 *   Refused   on the host, the context left usable (PG_ERR_INVALID): no rules (the reference indexes configs[len - 1], :123);
 *             ACCUMULATE counts that decrease along the list (the reference slices with a negative bound and panics, :193-195); a
 *             source named twice (the reference emits its items twice); PG_TRIM_ANY beside other rules; a source >=
 *             PG_TRIM_MAX_SOURCES; an unknown type; rules that name sources without d_source.  More than PG_TRIM_MAX_RULES rules
 *             and cap outside [1, PG_TRIM_MAX_CAP] are PG_ERR_UNSUPPORTED.
 *   Width     pg_trim_out_cap: a pure host function (no context, no device) that validates the rules as above and returns
 *             out_cap = min(cap, the sum of the FIX counts + the largest ACCUMULATE count) — no request can keep more.
 *   Kernel    one workgroup of PG_TRIM_CHUNK lanes per request: count the classes, plan takes and bases, walk the sorted order
 *             PG_TRIM_CHUNK positions at a time (an entry's rank within its class from wave ballots and per-wave class counts),
 *             pad.  Every output element is written exactly once.
 *   Stream    the score sort and one launch on the context's stream, no synchronisation (as pg_fanin_merge_dev). */
#define PG_TRIM_FIX 0
#define PG_TRIM_ACCUMULATE 1
#define PG_TRIM_ANY 0xFF
#define PG_TRIM_MAX_RULES 8
#define PG_TRIM_MAX_SOURCES 8
#define PG_TRIM_MAX_PLANES 8
#define PG_TRIM_MAX_CAP 16384
#define PG_TRIM_CHUNK 1024
typedef struct {
    uint8_t  source;   /* < PG_TRIM_MAX_SOURCES, or PG_TRIM_ANY */
    uint8_t  type;     /* PG_TRIM_FIX / PG_TRIM_ACCUMULATE */
    uint32_t count;
} pg_trim_rule;
int pg_trim_out_cap(const pg_trim_rule* rules, uint32_t n_rules, uint32_t cap, uint32_t* out_cap);
int pg_candidates_trim_dev(pg_ctx* ctx, const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                           const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                           uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                           double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                           float* d_out_planes_f32, uint32_t* d_out_count);

/* SnakeFilter and CompletelyFairCountFilter on the device (csrc/blend.hip): the two reference filters that sit in
 * the trim's slot, between UniqueFilter and RankService.Rank (service/user_recommend.go:105-137), and interleave the recalls
 * instead of cutting them.  SnakeFilter (filter/snake_filter.go:173-241) orders every configured recall by its own score and
 * deals them out round after round by weight; an item reached through a recall other than its first takes that recall's name
 * and score (:83-88) — the one filter that consumes RecallScores, i.e. the fan-in's per-recall score planes and source mask.
 * CompletelyFairCountFilter (filter/completely_fair_count_filter.go:34-94) sorts the merged list by score and deals the recalls
 * out one item at a time.
 *   In        pg_fanin_merge_dev's outputs as they are, in pg_candidates_trim_dev's argument order and optionality: nq <= 256
 *             requests of cap in [1, PG_BLEND_MAX_CAP] entries; d_rows, d_score, optional d_source, d_count, d_planes_f64
 *             [n_f64][nq][cap] (planes 0.. are the per-recall scores by source index), d_source_mask, d_planes_f32; at most
 *             PG_BLEND_MAX_PLANES planes each.  An entry is padding if its row is UINT64_MAX, its position is >= d_count[q] or
 *             its source is >= PG_BLEND_MAX_SOURCES; padding may sit anywhere, is dropped and never counted.  Without d_source
 *             every real entry belongs to one source (SNAKE: the single entry's).
 *   Conf      host values: mode, retain_num, and for the SNAKE modes n_entries <= PG_BLEND_MAX_SOURCES of {source, weight} in
 *             AdjustCountConfs order (source = the fan-in source index RecallName resolves to).  FAIR ignores the entries.
 *   Answer    DEFINED bit for bit.  "Score order" is pg_sort_scores_dev's: descending, -0.0 equals +0.0, NaN last, ties keep
 *             input position (the reference sorts unstably: only the order among equal keys is being fixed).
 *             SNAKE   entry i names source s_i; its list holds the real entries e with source[e] == s_i, key d_score[e]
 *                     (:63-67), and — with a mask — those with popcount(mask[e]) > 1, bit s_i of mask[e] set and source[e] !=
 *                     s_i, key planes_f64[s_i][e] (:188-200; the reference's len(RecallScores) > 1), each list in score order
 *                     of its key.  Entries of sources no entry names are dropped.  While size < retain_num a round runs
 *                     (:212-231): entry i = 0 .. n_entries - 1 advances through its list from its cursor and stops after
 *                     weight[i] slots (Next, :76-109); an entry nobody took yet is picked and costs a slot, one already taken
 *                     costs no slot under PG_BLEND_SNAKE_REFILL and one under PG_BLEND_SNAKE_SKIP, the cursor advances either
 *                     way; size += the round's picks; a round without a pick ends the walk (under SKIP even where fresh
 *                     entries lie further down: the reference's quirk, kept).  The output is the picks in pick order cut to
 *                     retain_num (:229-231).  A pick carries its row, score = its key in the picking list, source = s_i and
 *                     every carried plane, mask and fp32 plane unchanged.
 *             FAIR    retain = min(retain_num, the real entries); they are put in score order of d_score and grouped by
 *                     source, the names in order of first appearance (:59-65); while count < retain, slot count % len(names)
 *                     gives its next entry, and a name that has given its last entry is replaced by the last name, the list
 *                     shrinking by one (:80-83).  Scores and sources are unchanged.
 *             d_out_count[q] = the entries kept; behind them padding as the trim's: row UINT64_MAX, score -inf, source 0xFF,
 *             fp64 planes the quiet NaN 0x7FF8000000000000, mask 0, fp32 planes 0.  Outputs are [nq][out_cap] (planes
 *             [n][nq][out_cap]) with out_cap from pg_blend_out_cap; an output is required exactly where its input is given;
 *             outputs must not overlap inputs.  No value meets arithmetic: doubles and floats travel as bits.
 *   Refused   on the host, the context left usable (PG_ERR_INVALID): an unknown mode; retain_num == 0; SNAKE with no entries, a
 *             source >= PG_BLEND_MAX_SOURCES, a source named twice (the reference's map keeps only the later iterator) or every
 *             weight 0 (the reference divides 0 by 0 for its counts; one weight of 0 is legal: that recall never gives, and a
 *             weight above the list's length drains the list); a mask without the planes it needs (SNAKE: n_f64 must exceed
 *             every named source); SNAKE naming more than one source without d_source.  n_entries > PG_BLEND_MAX_SOURCES and
 *             cap outside [1, PG_BLEND_MAX_CAP] are PG_ERR_UNSUPPORTED.
 *   Width     pg_blend_out_cap: a pure host function (no context, no device) that validates the conf and returns out_cap =
 *             min(cap, retain_num).
 *   Host      pg_candidates_blend_host: the same answer computed on the host over host arrays (no context, no device) — the
 *             statement the device path is tested against, and the path of a host that holds the merged list already.
 *   Kernel    one workgroup per request.  FAIR: the trim's score sort, then counts and first appearances per source, a plan of
 *             at most 8 phases between exhaustions by one lane, and every entry's output position from its rank within its
 *             source — no loop over retain.  SNAKE: one sorted order per entry (keys built per entry, non-members NaN), each
 *             list compacted to its members in order, then one wave walks (round, entry) steps 64 list entries at a time
 *             against a bitmap of taken positions in LDS and records the picks, which the whole workgroup gathers.  Every
 *             output element is written exactly once.  The snake_filter debug property (:89-99,232-236) is not built.
 *   Stream    the sorts and the launches on the context's stream, no synchronisation (as pg_candidates_trim_dev). */
#define PG_BLEND_SNAKE_REFILL 0   /* SnakeType default, REFILL_ON_DUPLICATE */
#define PG_BLEND_SNAKE_SKIP   1   /* SnakeType "SKIP_ON_DUPLICATE" */
#define PG_BLEND_FAIR         2   /* CompletelyFairCountFilter */
#define PG_BLEND_MAX_SOURCES  8   /* == PG_FANIN_MAX_SOURCES */
#define PG_BLEND_MAX_PLANES   8
#define PG_BLEND_MAX_CAP      16384   /* == PG_FANIN_MAX_CAP */
typedef struct {
    uint32_t mode, retain_num, n_entries;          /* n_entries: SNAKE only (AdjustCountConfs, in config order) */
    uint8_t  source[PG_BLEND_MAX_SOURCES];         /* the fan-in source index entry i names */
    uint32_t weight[PG_BLEND_MAX_SOURCES];
} pg_blend_conf;
int pg_blend_out_cap(const pg_blend_conf* conf, uint32_t cap, uint32_t* out_cap);
int pg_candidates_blend_dev(pg_ctx* ctx, const pg_blend_conf* conf, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                            const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                            uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                            double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                            float* d_out_planes_f32, uint32_t* d_out_count);
int pg_candidates_blend_host(const pg_blend_conf* conf, uint32_t nq, uint32_t cap, const uint64_t* rows, const double* score,
                             const uint8_t* source, const uint32_t* count, const double* planes_f64, uint32_t n_f64,
                             const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32, uint64_t* out_rows, double* out_score,
                             uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32,
                             uint32_t* out_count);

/* PriorityAdjustCountFilterV2 on the device (csrc/trim2.hip): the quota filter of a scene whose recalls overlap
 * (filter/priority_adjust_count_filter_v2.go:39-103, registered in filter/filter.go:148), in the trim's slot between UniqueFilter
 * and RankService.Rank (service/user_recommend.go:105-137).  An item that several recalls returned counts for every one of them,
 * under that recall's score (RecallScores, i.e. the fan-in's per-recall score planes and source mask), until one quota takes it;
 * it then leaves with that recall's name and score.  pg_candidates_trim_dev treats an item as its first recall's only: on
 * overlapping recalls that is a different answer.
 *   In        pg_fanin_merge_dev's outputs as they are, in pg_candidates_trim_dev's argument order and optionality: nq <= 256
 *             requests of cap in [1, PG_TRIM_MAX_CAP] entries; d_rows, d_score, optional d_source, d_count, d_planes_f64
 *             [n_f64][nq][cap] (planes 0.. are the per-recall scores by source index), d_source_mask, d_planes_f32; at most
 *             PG_TRIM_MAX_PLANES planes each.  An entry is padding if its row is UINT64_MAX or its position is >= d_count[q];
 *             padding may sit anywhere, is dropped and never counted.
 *   Rules     host values, 1 .. PG_TRIM_MAX_RULES of pg_trim_rule {source, type, count} in AdjustCountConfs order: type
 *             PG_TRIM_FIX or PG_TRIM_ACCUMULATE, source < PG_TRIM_MAX_SOURCES (the fan-in source index RecallName resolves to).
 *   Answer    DEFINED bit for bit.  "Score order" is pg_sort_scores_dev's: descending, -0.0 equals +0.0, NaN last, ties keep
 *             input position (the reference shuffles and sorts unstably, :47-52, and iterates a Go map, :66: only the order
 *             among equal keys is being fixed).
 *               1. a real entry e is a duplicate iff a mask is given and popcount(mask[e]) > 1 (the reference's
 *                  len(RecallScores) > 1, :55); otherwise it is a single.
 *               2. rule c names source s_c; its list L_c holds the singles with source[e] == s_c, keyed d_score[e] (:58,63), and
 *                  every duplicate with bit s_c of mask[e] set, keyed planes_f64[s_c][e] — also where source[e] == s_c (:66-71:
 *                  RecallScores[name] is read for every name; it differs from Item.Score only where the first recall held the
 *                  id twice, unique_filter.go:40-43).  L_c is in score order of its key.  Without d_source the single legal
 *                  rule owns every entry: each real entry counts as of source s_0.
 *                  Singles of sources no rule names, and duplicates no named source holds, are dropped.
 *               3. rules apply in order with acc = 0 and taken empty: limit_c = count_c for PG_TRIM_FIX, max(0, count_c - acc)
 *                  for PG_TRIM_ACCUMULATE (:86); the picks are the first limit_c entries of L_c that are not in taken, in
 *                  order — an entry an earlier rule took does not use up a place (the reference deletes it from the map,
 *                  :80-83,91-93; pg_candidates_classcut_dev's window differs in this); taken gains the picks; an ACCUMULATE
 *                  rule adds their number to acc (:95), a FIX rule leaves acc alone.
 *               4. the output is the picks concatenated in rule order.  A pick carries its row, score = its key in L_c, source
 *                  = s_c (:68-69) and every plane, mask and fp32 plane unchanged; doubles and floats travel as bits.
 *                  d_out_count[q] = the picks; behind them padding as the trim's: row UINT64_MAX, score -inf, source 0xFF, fp64
 *                  planes the quiet NaN 0x7FF8000000000000, mask 0, fp32 planes 0.
 *             Outputs are [nq][out_cap] (planes [n][nq][out_cap]) with out_cap from pg_trim2_out_cap; an output is required
 *             exactly where its input is given.  Without a mask every entry is a single and the answer equals
 *             pg_candidates_trim_dev's on the same rules, bit for bit.
 *   Refused   on the host, the context left usable (PG_ERR_INVALID): no rules; a source named twice (the reference emits its
 *             singles twice); PG_TRIM_ANY; a source >= PG_TRIM_MAX_SOURCES; an unknown type; a mask without planes covering every
 *             named source (n_f64 must exceed every named source); more than one source named without d_source; an output
 *             missing where its input is given; an output that overlaps its input.  ACCUMULATE counts that decrease are legal
 *             here: V2 compares (i < count, :88) where v1 slices and panics.  More than PG_TRIM_MAX_RULES rules and cap outside
 *             [1, PG_TRIM_MAX_CAP] are PG_ERR_UNSUPPORTED.
 *   Width     pg_trim2_out_cap: a pure host function (no context, no device) that validates the rules as above and returns
 *             out_cap = min(cap, the sum of the FIX counts + the largest ACCUMULATE count), computed in 64 bits: acc never
 *             exceeds the largest ACCUMULATE count and a position is picked once.
 *   Host      pg_candidates_trim2_host: the same answer computed on the host over host arrays (no context, no device) — the
 *             statement the device path is tested against, and the path of a host that holds the merged list already.
 *   Kernel    one key array per rule (non-members NaN), one segmented score sort over nq x n_rules segments, then one workgroup
 *             of PG_TRIM_CHUNK lanes per request: rules one after another, each walking its order PG_TRIM_CHUNK positions at a
 *             time against a bitmap of taken input positions in LDS (an eligible entry's rank from wave ballots and per-wave
 *             counts), until its picks reach the limit or the order ends.  Every output element is written exactly once.
 *   Stream    the sort and the launches on the context's stream, no synchronisation (as pg_candidates_trim_dev).
 * Not served here: AdjustCountConfig's Expression / Weight (V2 does not read them). */
int pg_trim2_out_cap(const pg_trim_rule* rules, uint32_t n_rules, uint32_t cap, uint32_t* out_cap);
int pg_candidates_trim2_dev(pg_ctx* ctx, const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                            const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                            uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                            double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                            float* d_out_planes_f32, uint32_t* d_out_count);
int pg_candidates_trim2_host(const pg_trim_rule* rules, uint32_t n_rules, uint32_t nq, uint32_t cap, const uint64_t* rows,
                             const double* score, const uint8_t* source, const uint32_t* count, const double* planes_f64, uint32_t n_f64,
                             const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32, uint64_t* out_rows, double* out_score,
                             uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32,
                             uint32_t* out_count);

/* Refresh: bring an existing index back to its table's current rows KEEPING ITS CENTROIDS — cheap when few
 * rows were written, several times cheaper than pg_index_build when all of them were (nothing is trained).  Nothing changes
 * until it is called: a written table still makes its index stale.
 *   Exact     after a refresh every recall through the index, attached or not, filtered or not, is bit for bit the table's pass
 *             on the current rows, as after a build: every radius is measured anew over the rows of the new lists.
 *   Rule      a row's list is the one the build's assignment gives it for the kept centroids (the smallest cn2[L] - 2 x.c_L in
 *             the build's fp32 chains, ties to the lower list, a NaN row to list 0), whichever mode ran: pg_index_read afterwards
 *             equals what the build's sort, offsets and radius steps produce for these centroids and rows; centroids and cnorm are
 *             unchanged; a forced full refresh of an unchanged table reproduces the built arrays.
 *   Modes     incremental: only the rows in the table's write log are re-assigned (the log: at most 64 disjoint row ranges that
 *             pg_table_upload wrote since some generation; pg_table_fill_*, pg_table_swap, a 65th range and more than
 *             "index_refresh_full_fraction" of the rows — the option of the context that uploads — reset it).  full: every row, on the bf16 matrix pipe as a rigorous screen
 *             with the surviving lists confirmed by the rule's own chain (dim 64 / 128; rows it cannot settle, and dim 192 / 256,
 *             go through the build's fp32 kernel).  mode 0 picks incremental when the log covers every write since the index's
 *             generation and holds at most that fraction of the rows, else full; mode 1 is full; mode 2 is incremental, or
 *             PG_ERR_UNSUPPORTED (the index unchanged) when the log does not reach back.  A current index is left alone
 *             (`noop`) unless force != 0 (then mode 0 / 1 refresh in full).
 *   Install   the new arrays are built in new device memory under the table's shared lock (other contexts keep serving through
 *             the table's pass), then exchanged as pg_index_attach replaces an index: the table's lock exclusively, no generation
 *             bump, the device drained.  The index then describes the generation read under the shared lock: a write in
 *             between leaves it stale again.  Its filtered lists' cache is dropped.  An attached index stays attached, its
 *             counters go on.  Any context may call it; refreshes of one index are serialised.
 *   Context   the calling context is busy for the whole refresh (seconds at 100 M rows: every other call on it, a coalescer
 *             created on it included, waits): refresh from the loader's context, not from the one that serves.
 *   Errors    PG_ERR_INVALID for a NULL ctx / ix or an unknown mode; PG_ERR_NOMEM / PG_ERR_DEVICE leave the index as it was,
 *             stale and valid.  A refresh holds about 24 B per row of device memory beside the index while it runs (the new
 *             permutation, three row-sized work arrays, the sort's 8 B per row: 2.4 GB at 100 M rows) plus a 128 MB gather buffer.
 * pg_index_stats reports the refreshed generation, radii, largest_list and empty_lists afterwards; build_ms stays the build's. */
typedef struct {
    int      mode;        /* 0 = auto, 1 = full, 2 = incremental or PG_ERR_UNSUPPORTED */
    int      force;       /* != 0: refresh even when the index is current */
} pg_index_refresh_params;                       /* NULL = {0, 0} */
int pg_index_refresh(pg_ctx* ctx, pg_index* ix, const pg_index_refresh_params* p);
typedef struct {
    uint64_t refreshes, full, incremental, noop;  /* calls by what they did (noop: the index was current and force == 0) */
    uint64_t rows_reassigned;                     /* rows whose list was recomputed, summed */
    uint64_t rows_moved;                          /* ... of which the list changed */
    uint64_t rows_confirmed_wide;                 /* full refreshes: rows that left the matrix-pipe screen for the fp32 kernel */
    uint64_t last_generation;                     /* the table generation the index describes now */
    double   last_ms, last_assign_ms;             /* wall time of the last refresh, device time of its assignment */
} pg_index_refresh_stats_t;
int pg_index_refresh_stats(const pg_index* ix, pg_index_refresh_stats_t* out);
/* Diagnostic of the full refresh's matrix-pipe screen: for host rows [n][dim] and centroids [n_lists][dim]
 * (dim 64 / 128, n and n_lists <= 65536) out_s[row][L] is the screen's distance — the same loads, MFMA sequence and formulas as
 * the assignment — and out_e[row][L] the bound e(x, L) the kernel applies to it, +inf where the row or the centroid lies
 * outside the range the bound is claimed for.  |out_s - (cn2[L] - 2 x.c_L in the build's fp32 chains)| <= out_e is what the
 * equality of the two refresh modes rests on; tests check it on the device.  PG_ERR_INVALID for NULLs, dim or sizes. */
int pg_index_screen_probe(pg_ctx* ctx, uint32_t dim, const float* rows, uint32_t n, const float* centroids, uint32_t n_lists,
                          float* out_s, float* out_e);
/* FM + two-tower rank straight from candidate rows: the model's item field ids are the integer columns
 * item_field_cols[n_item_fields] of `fs`.
 * THE CLAMP ON ITEM IDS: an item field id is the column's value saturated to int32 (as pg_features_gather_i32_dev), then clamped
 * to [0, vocab - 1] — -1 reads id 0, `vocab` and 2^40 read id vocab - 1.  pg_rank_fm2t_dev (device ids), this call and the item
 * records (pg_fm2t_item_rows_*) apply the same rule and score an out-of-vocabulary id bit for bit as the clamped id; only the
 * host entry pg_rank_fm2t, which sees the ids, refuses them (PG_ERR_INVALID names the first). */
int pg_rank_fm2t_rows_dev(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                          const float* d_user_vecs, const int32_t* d_user_field_ids, const uint32_t* d_cand_rows,
                          const uint32_t* d_req_offsets, uint32_t n_req, uint32_t n_items, float* d_out_scores);

/* host-buffer form of the same: the EasyRec flavour of IAlgorithm.Run (service/rank/algo_data.go:79-86: item ids + columnar
 * context features) with the columns already resident — the shim passes candidate rows, nothing is boxed per request */
int pg_rank_fm2t_rows(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                      const float* user_vecs, const int32_t* user_field_ids, const uint32_t* cand_rows,
                      const uint32_t* req_offsets, uint32_t n_req, float* out_scores);

/* ---- materialised item records (FM + two-tower) ---------------------------------------------------------------
 * An item's field ids are static per item (the columns of `fs`), so the item side of model `m` can be laid out once, at
 * model-load / column-set time: record r = the embeddings of row r's ids concatenated in field order (128 fp32) followed
 * by their linear weights — 640 B, ONE contiguous gather per candidate at rank time instead of the id row plus
 * n_item_fields scattered 64-B embedding rows (each of which costs a whole 128-B line of HBM traffic).  The records
 * hold the very values the per-field path reads and the kernel sums them in the same order, so scores are bit-identical
 * to pg_rank_fm2t_rows_dev in both precision modes; candidates outside the store read the columns' defaults as there.
 * After a column changes (pg_features_set_column) or the model's field tables are reloaded, _update re-materialises
 * rows [row0, row0 + nrows) and always the defaults' record (nrows = 0 refreshes that alone); a range that does not lie
 * inside the store — row0 > rows or nrows > rows - row0, a row0 + nrows that wraps included — is PG_ERR_INVALID with nothing
 * launched.  The per-field path stays available for field-table hot-swaps. */
typedef struct pg_item_rows pg_item_rows;
int pg_fm2t_item_rows_build(pg_ctx* ctx, const pg_model* m, const pg_features* fs, const int32_t* item_field_cols,
                            pg_item_rows** out);
int pg_fm2t_item_rows_update(pg_ctx* ctx, pg_item_rows* ir, uint64_t row0, uint64_t nrows);
int pg_fm2t_item_rows_destroy(pg_ctx* ctx, pg_item_rows* ir);
/* pg_rank_fm2t_rows_dev / pg_rank_fm2t_rows over the materialised records */
int pg_rank_fm2t_irows_dev(pg_ctx* ctx, const pg_model* m, const pg_item_rows* ir, const float* d_user_vecs,
                           const int32_t* d_user_field_ids, const uint32_t* d_cand_rows, const uint32_t* d_req_offsets,
                           uint32_t n_req, uint32_t n_items, float* d_out_scores);
int pg_rank_fm2t_irows(pg_ctx* ctx, const pg_model* m, const pg_item_rows* ir, const float* user_vecs,
                       const int32_t* user_field_ids, const uint32_t* cand_rows, const uint32_t* req_offsets, uint32_t n_req,
                       float* out_scores);

/* ---- the whole hot path in one call ------------------------------------------------------------
 * One request batch through VectorRecall.GetCandidateItems → RankService.Rank (one DNN3 rank algorithm) →
 * RankScore fusion → ItemRankScoreSort (service/user_recommend.go:83-151 restricted to the hot path),
 * device-resident: recall top-k of `t` for nq user vectors, rank every candidate with `m` (the same user
 * vectors are the model's user features), fuse with `e` — whose variables must be `rank_var` (the model's
 * name in RankAlgoList) and/or "current_score" (Item.Score, i.e. the recall score, module/item.go:189-212) —
 * and sort each request's candidates by the fused score, descending.
 * Outputs, all [nq][k]: global row ids and recall scores in recall order, the model's scores, the fused fp64
 * scores (same order), and d_out_order = positions 0..k-1 of each request sorted by fused score.
 * d_out_count (optional, [nq]) receives each request's number of real candidates: a table with fewer than k rows
 * pads every list with row = UINT64_MAX, recall score = -inf, model score = 0, fused score = NaN — the sort puts
 * those slots last, so the first d_out_count[q] positions of a request's order are its items.
 * The stages are enqueued back to back and verified once, at the end; the call returns after that check. */
int pg_recommend_dnn3_dev(pg_ctx* ctx, const pg_table* t, const pg_model* m, const pg_expr* e, const char* rank_var,
                          const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                          float* d_out_recall_scores, float* d_out_rank_scores, double* d_out_fused,
                          uint32_t* d_out_order, uint32_t* d_out_count);

/* The same batch in two halves, for callers that keep several batches queued on the stream (bench.py; a serving loop
 * that owns its batching): _begin enqueues everything and returns at once with a ticket, _end waits for that batch,
 * verifies it (re-running it with the fallback recall plan if the first one did not hold) and frees the ticket.
 * Every ticket must be ended; output buffers belong to the batch until then. */
typedef struct pg_ticket pg_ticket;
int pg_recommend_dnn3_begin(pg_ctx* ctx, const pg_table* t, const pg_model* m, const pg_expr* e, const char* rank_var,
                            const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_rows,
                            float* d_out_recall_scores, float* d_out_rank_scores, double* d_out_fused,
                            uint32_t* d_out_order, uint32_t* d_out_count, pg_ticket** out);
/* scan_ms (optional): the batch's scan-stage launches, HIP-event timed (what pg_last_scan_kernel_ms reports) */
int pg_recommend_end(pg_ctx* ctx, pg_ticket* ticket, double* scan_ms);

/* The stages behind the recall for candidate lists the caller made — the merged answer of several recalls
 * (pg_fanin_merge_dev: service/recall.go:126-150 + filter/unique_filter.go:26-49), or any other [nq][cap] lists: rank every
 * candidate with the DNN3 `m` → ScoreRewrite / RankScore fusion → ItemRankScore sort, as pg_recommend_dnn3_dev runs them
 * behind its vector recall, with one version of the table for the whole call.
 *   In        d_rows [nq][cap] global row ids of `t` (UINT64_MAX = padding; a row outside `t` counts as padding), d_score
 *             [nq][cap] fp64 — Item.Score, what "current_score" binds to, with all 64 bits — d_count [nq] (optional: slots from
 *             d_count[q] on are padding whatever they hold), d_user_vecs [nq][dim]; 1 <= nq <= 256, 1 <= cap <= 16384; model,
 *             expression and rank_var as pg_recommend_dnn3_dev.  These are pg_fanin_merge_dev's d_out_rows / d_out_score /
 *             d_out_count as they are.
 *   Out       all [nq][cap]: the model's scores, the fused fp64 scores, d_out_order = each request's positions sorted by fused
 *             score, descending.  Padding slots: model score 0, fused NaN, last in the order.  Fed one vector recall's [nq][k]
 *             answer with its scores widened, the three outputs are bit for bit pg_recommend_dnn3_dev's.
 *   Errors    a filtered view is refused (PG_ERR_UNSUPPORTED) as there; PG_ERR_ARITH when the RankScore divides by zero.  The
 *             call returns synchronised.
 * Not served here yet: the coalescer, scenes, the shard group, a DPP stage behind the sort and the _begin / _end ticket form.
 * (An SSDSort stage behind the sort is pg_ssd_sort_dev: it takes d_out_order, d_out_fused and d_rows as they are.) */
int pg_recommend_candidates_dnn3_dev(pg_ctx* ctx, const pg_table* t, const pg_model* m, const pg_expr* e, const char* rank_var,
                                     const float* d_user_vecs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                                     const double* d_score, const uint32_t* d_count, float* d_out_rank_scores,
                                     double* d_out_fused, uint32_t* d_out_order);

/* The coarse-rank cascade over candidate lists the caller made: GeneralRank
 * (service/general_rank/base_general_rank.go:66-238, action.go:61-83) in front of RankService.Rank, as
 * service/user_recommend.go:105-137 runs them, in one call with one version of the table:
 *   1. the coarse DNN3 `m_coarse` scores all cap candidates of every request;
 *   2. the `e_coarse` fusion: variables `coarse_var` and/or "current_score" (d_score); its fp64 result becomes Item.Score
 *      (base_general_rank.go:221-227);
 *   3. ItemRankScore sorts each request by it, descending;
 *   4. pg_candidates_trim_dev's kernel with the single rule {PG_TRIM_ANY, PG_TRIM_FIX, n_keep} keeps the first n_keep
 *      (AdjustCountFilter, ShuffleItem false), carrying rows, the coarse fused score, the source and the coarse model score;
 *   5. the fine DNN3 `m_fine` scores the survivors;
 *   6. the `e_fine` fusion: variables `fine_var`, `coarse_var` — the carried coarse model score, still in the item's
 *      algoScores (module/item.go:168-212) — and/or "current_score", now the coarse fused fp64 score;
 *   7. ItemRankScore sorts the survivors by the fine fused score, descending.
 *   In        as pg_recommend_candidates_dnn3_dev (d_rows, d_score, d_count optional, d_user_vecs; padding = row UINT64_MAX, a
 *             row outside `t`, a slot from d_count[q] on) plus d_source [nq][cap] uint8 (optional); 1 <= n_keep <= cap <= 16384;
 *             both models DNN3 with one output and d_user = d_item = the table's dim; fine_var and coarse_var must differ
 *             (PG_ERR_INVALID).
 *   Out       [nq][n_keep]: d_out_rows, d_out_coarse_fused (fp64), d_out_source (required iff d_source is given),
 *             d_out_model_scores [2][nq][n_keep] float — plane 0 the fine model's scores, plane 1 the coarse model's —,
 *             d_out_fused (fp64, the fine fusion), d_out_order = each request's positions 0 .. n_keep - 1 sorted by d_out_fused;
 *             d_out_count [nq] = the survivors.  The coarse stage leaves padding with a NaN score, which sorts last: survivors are
 *             real candidates as long as there are any, then rows outside `t` (counted, and padding again for the fine stage),
 *             never UINT64_MAX rows or slots beyond d_count.  Slots behind d_out_count[q]: row UINT64_MAX, coarse fused -inf,
 *             source 0xFF; padding of the fine stage has model scores 0, fused NaN and is last in the order, as in
 *             pg_recommend_candidates_dnn3_dev.
 *   Same as   the stages run one by one: pg_recommend_candidates_dnn3_dev with the coarse model, the trim, pg_rank_dnn3 on the
 *             surviving rows (model scores and everything carried are bit-identical).
 *   Errors    a filtered view is refused (PG_ERR_UNSUPPORTED); PG_ERR_ARITH when either RankScore divides by zero.  The call
 *             returns synchronised.
 * Not served here yet: what pg_recommend_candidates_dnn3_dev does not serve, an FM + two-tower coarse model and the filter's
 * diversity branch (ensureDiversity, DiversityDao).  (PriorityAdjustCountFilterV2 is pg_candidates_trim2_dev.) */
int pg_recommend_cascade_dnn3_dev(pg_ctx* ctx, const pg_table* t, const pg_model* m_coarse, const pg_expr* e_coarse,
                                  const char* coarse_var, const pg_model* m_fine, const pg_expr* e_fine, const char* fine_var,
                                  const float* d_user_vecs, uint32_t nq, uint32_t cap, const uint64_t* d_rows, const double* d_score,
                                  const uint8_t* d_source, const uint32_t* d_count, uint32_t n_keep, uint64_t* d_out_rows,
                                  double* d_out_coarse_fused, uint8_t* d_out_source, float* d_out_model_scores, double* d_out_fused,
                                  uint32_t* d_out_order, uint32_t* d_out_count);

/* DiversityRuleSort on the device (csrc/diversity.hip): the windowed scatter rules that follow ItemRankScore
 * in most scenes (sort/diversity_rule_sort.go:116-283, sort/diversity_rule.go:50-92, sort/diversity_exclusion_rule.go:37-56),
 * for nq <= 256 requests of cap <= PG_DIV_MAX_N candidates each, without leaving device memory.
 *   In        a request's candidates in the order the previous sort left them; position 0 .. n - 1 is an entry's identity.
 *             (The reference's alreadyMatchItems, :156, is keyed by item id; after UniqueFilter ids are unique, so a "taken"
 *             flag per position is the same thing.)  dims [n_cols][nq][cap] int64: column c of the entry at position i of
 *             request q is dims[(c * nq + q) * cap + i] — dictionary codes or integer features; source [nq][cap] uint8
 *             (Item.RetrieveId as fan-in numbers it; optional), count [nq] (optional: cap), enable [nq] bytes (optional: the
 *             sort's Conditions gate, :74-85, evaluated by the caller; 0 = the request's order is the identity).
 *   Config    host values: size = ctx.Size, diversity_size / explore_item_size (<= 0: off, :46-48) / exclude_source_mask (bit s:
 *             source s is among ExcludeRecalls; sources >= 32 are never excluded), 0 .. PG_DIV_MAX_RULES rules {1 ..
 *             PG_DIV_MAX_DIMS column indices, interval, window, frequency, weight} and 0 .. PG_DIV_MAX_EXCL exclusion rules
 *             {1-based positions, 1 .. PG_DIV_MAX_TERMS terms `column OP value` (pg_where_op), all ANDed}.
 *   Values    a rule's value for an entry is the TUPLE of its dimension columns; two values are equal iff every column is.
 *             The reference joins the columns' strings with "_" (diversity_rule.go:45), so ("a_b", "c") equals ("a", "b_c")
 *             there and not here; a caller who wants that encodes the joined string as one column.
 *   Match     (diversity_rule.go:50-92) with s results so far, an entry FAILS rule r when interval > 0, s >= interval and the
 *             last `interval` results all carry its value (:54-69), or when window > 0, frequency > 0, window > frequency and
 *             1 + the results in [max(0, s - window + 1), s) that carry its value > frequency (:71-90).
 *             An exclusion rule matches (position, entry) iff the position is among its positions and every term holds.
 *   Answer    DEFINED bit for bit (doSort, :116-283): no rules, enable == 0 or nothing left after the set-aside → identity.
 *             Else the entries whose source is in exclude_source_mask are set aside in order (:127-138; the m others are
 *             renumbered 0 .. m - 1 in order, and distances below are in that numbering); D = size, or min(diversity_size, m)
 *             when diversity_size > 0 (:146-153).  First pick: the first entry no exclusion rule matches at position 1, entry
 *             0 if all match or there are no exclusion rules (:158-184).  Then while len(result) <= D — note <=: up to D + 1
 *             greedy picks, :197 — and picks != m (:198): walk the untaken entries in order, skipping those an exclusion rule
 *             matches at position len(result) + 1 (:210-221); f = the first entry not skipped; the walk stops at an entry i
 *             with explore_item_size > 0 and i - f >= explore_item_size (:226, taken entries count); if any rule has weight >
 *             0 every rule is evaluated and w = the sum of the weights of the rules that do not fail (:231-238), else the
 *             entry passes iff no rule fails; the first entry that passes every rule is taken (:246-250); if none does, the
 *             evaluated entry with the largest w, the first one on ties (:256-265, :302-310; without weights: the first
 *             evaluated entry); if every untaken entry was skipped the loop ends (:266).  Output: the result, the untaken
 *             entries in order (:271-276), the set-aside entries in order (:278) — a permutation of 0 .. n - 1 as uint32
 *             positions; slots at positions >= count receive UINT32_MAX.
 *   Refused   on the host, the context left usable.  PG_ERR_INVALID: a rule's n_dims 0 or > PG_DIV_MAX_DIMS, a column index >=
 *             n_cols, a negative interval / window / frequency, an unknown operator, a position of 0, an exclusion rule with
 *             no term or no position, exclude_source_mask without source.  No rules is NOT an error (identity, :121-123).
 *             PG_ERR_UNSUPPORTED: more rules / exclusion rules / terms / columns than the limits, cap > PG_DIV_MAX_N, nq >
 *             256, more than PG_DIV_MAX_POSITIONS reachable positions (<= PG_DIV_MAX_N + 1) in one exclusion rule, and
 *             n_multi_value > 0: MultiValueDimensionConf (list-valued dimensions, diversity_rule.go:101-210) is not served.
 *             Exclusion terms that are not integer comparisons cannot be expressed here; the host mirror refuses them by name.
 *   host      pg_diversity_rules_host: a pure host function (no context, no device) that validates the config and states
 *             what the kernel reproduces; tests compare the kernel with it.  The library falls back to it for nothing.
 *   dev       pg_diversity_rules_dev: the same over device arrays, one launch on the context's stream, no synchronisation.
 *   features  pg_diversity_rules_features_dev: column c is the int32 / int64 column col_names[c] of fs at the candidates'
 *             rows d_rows [nq][cap] uint64 (a row outside the store reads the column default), gathered into planes in context
 *             scratch; then the same kernel.  A float column, a column without values or an unknown name is PG_ERR_INVALID.
 *   one       pg_diversity_rules: host arrays of one request, dims [n_cols][n] (upload, run, download, synchronise).
 *   Kernel    one workgroup of PG_DIV_CHUNK lanes per request.  Prepare: the set-aside compaction; per rule an exact key per
 *             entry = the first entry with an equal tuple, through an open-addressed table in which tuples themselves are
 *             compared (no hash ever stands for a tuple); one bit per (exclusion rule, entry).  Greedy: the taken bitmap, the
 *             result, the run of equal values at its tail and the count of every value inside the window per rule; a step
 *             scans PG_DIV_CHUNK entries at a time, one lane per entry against all rules, wave ballots and a scan of the
 *             waves' masks give the first passing entry, (largest w, first position) is carried across chunks, the explore
 *             bound ends the scan.  Every output element is written exactly once. */
#define PG_DIV_MAX_N 8192
#define PG_DIV_MAX_RULES 8
#define PG_DIV_MAX_DIMS 4
#define PG_DIV_MAX_COLS 16
#define PG_DIV_MAX_EXCL 8
#define PG_DIV_MAX_TERMS 4
#define PG_DIV_MAX_POSITIONS 64
#define PG_DIV_CHUNK 1024
typedef struct {
    uint32_t n_dims;                    /* 1 .. PG_DIV_MAX_DIMS (DiversityRuleConfig.Dimensions) */
    uint32_t dims[PG_DIV_MAX_DIMS];     /* column indices < n_cols */
    int32_t  interval;                  /* IntervalSize */
    int32_t  window;                    /* WindowSize */
    int32_t  frequency;                 /* FrequencySize */
    int32_t  weight;                    /* Weight */
} pg_div_rule;
typedef struct {
    uint32_t  column;                   /* < n_cols */
    int32_t   op;                       /* pg_where_op */
    long long value;
} pg_div_term;
typedef struct {
    const uint32_t* positions;          /* ExclusionRuleConfig.Positions, 1-based */
    uint32_t        n_positions;
    uint32_t        n_terms;            /* 1 .. PG_DIV_MAX_TERMS (Conditions), all ANDed */
    pg_div_term     terms[PG_DIV_MAX_TERMS];
} pg_div_exclusion;
typedef struct {
    int32_t          size;              /* ctx.Size */
    int32_t          diversity_size;    /* DiversitySize; <= 0: off */
    int32_t          explore_item_size; /* ExploreItemSize; <= 0: off */
    uint32_t         exclude_source_mask;
    uint32_t         n_cols;            /* planes in dims, <= PG_DIV_MAX_COLS */
    uint32_t         n_rules;
    uint32_t         n_excl;
    uint32_t         n_multi_value;     /* MultiValueDimensionConf entries: anything but 0 is refused */
    pg_div_rule      rules[PG_DIV_MAX_RULES];
    pg_div_exclusion excl[PG_DIV_MAX_EXCL];
} pg_div_config;
int pg_diversity_rules_host(const pg_div_config* cfg, uint32_t nq, uint32_t cap, const uint32_t* count, const int64_t* dims,
                            const uint8_t* source, const uint8_t* enable, uint32_t* order);
int pg_diversity_rules_dev(pg_ctx* ctx, const pg_div_config* cfg, uint32_t nq, uint32_t cap, const uint32_t* d_count,
                           const int64_t* d_dims, const uint8_t* d_source, const uint8_t* d_enable, uint32_t* d_order);
int pg_diversity_rules_features_dev(pg_ctx* ctx, const pg_div_config* cfg, const pg_features* fs, const char* const* col_names,
                                    uint32_t nq, uint32_t cap, const uint64_t* d_rows, const uint32_t* d_count,
                                    const uint8_t* d_source, const uint8_t* d_enable, uint32_t* d_order);
int pg_diversity_rules(pg_ctx* ctx, const pg_div_config* cfg, uint32_t n, const int64_t* dims, const uint8_t* source,
                       uint32_t* order);

/* module.FilterParam as a compiled condition set, ItemStateFilter and BoostScoreSort on the device (DESIGN.md 4.1p;
 * csrc/cond.hip).  ItemStateFilter (filter/item_state_filter.go:47-57, module/item_state_filter_hologres_dao.go:86-357) keeps, in
 * order, the candidates whose state columns pass one FilterParam; BoostScoreSort (sort/boost_score_sort.go:73-104) rewrites
 * Item.Score by the expression of the first BoostScoreCondition whose FilterParam matches, or of every matching one in sequence
 * (BoostScoreConditionsFilterAll).  Both are one small program of `name OP value` operators (module/filter_op.go:453-540) per
 * candidate over columns keyed by item row.
 *   Rules     1 .. PG_COND_MAX_RULES rules; a rule is one FilterParam: 0 .. PG_COND_MAX_TERMS operators in the order given, all
 *             ANDed (EvaluateByDomain, :507-540; none: true, :539).  A `bool` operator (one level, :1679-1756) is followed by
 *             its children, which carry depth 1 and count among the rule's operators: bool_and == 0 (Type "" / "or") → any
 *             child, no children false; bool_and != 0 → every child, no children true.
 *   Terms     {name, domain "item" | "user" ("" = item, as the constructors do), op, type, right-hand side}.  Types: int and
 *             int64 on int32 / int64 columns (compared as int64: Go's int is 64-bit), float on any numeric column (compared as
 *             float64(value)), string for equal / not_equal / in / not_in over dictionary ids the caller encoded (integer
 *             columns).  Right-hand side: a constant (i, or f for float), user.<rhs_name>, item.<rhs_name> (another column), or
 *             for in / not_in a constant list of <= PG_COND_MAX_LIST values (sorted here, searched on the device).
 *   Binding   item names are columns DECLARED at compile {name, dtype} and bound by name to a pg_features store at run time
 *             (the store's dtype must be the declared one: PG_ERR_INVALID); only referenced columns are read, at most
 *             PG_COND_MAX_COLS.  User names become user slots in order of first use (pg_cond_user_slot_name), at most
 *             PG_COND_MAX_SLOTS: per request one 8-byte value per slot — int64, or fp64 when the terms that read it are float
 *             (pg_cond_user_slot_is_float; both is PG_ERR_INVALID) — and one presence bit per slot.
 *   Missing   the reference's "property missing from the map" branch is taken for a candidate whose row is outside the store
 *             (row >= the store's rows: the ItemStateFilter item absent from the state table, :313-340 of the DAO with empty
 *             defaultFieldValues — column defaults are NOT read) and for a user slot whose presence bit is clear.  Answers,
 *             from the form EvaluateByDomain dispatches to (DomainEvaluate; Evaluate for is_null / is_not_null):
 *               left missing      not_equal → true (:231-234), is_null → true (:1588-1596), every other operator false
 *                                 (:85-88, :356-359, :597-600, :771-774, :945-948, :1119-1122, :1492-1495, :1621-1626)
 *               type not listed   equal / not_equal with float → false (:167-169, :310-312); in / not_in with int64 or float
 *                                 → false (:420, :1562), whether the property is there or not
 *               user.x missing    equal false (:98-101), not_equal true (:244-247), ordered comparisons false (:610-613 ...)
 *               item.x missing    equal false (:106-109), not_equal true (:252-255), ordered comparisons TRUE for float
 *                                 (:618-621, :792-795, :966-969, :1140-1143) and false for int / int64 (:643-646 ...)
 *   Refused   by name at compile, nothing allocated.  PG_ERR_UNSUPPORTED: contains / not_contains (list-valued properties);
 *             expression (expr-lang); ordered comparisons on string; int / int64 / string terms on float columns (utils.ToInt
 *             has no float32 case and truncates float64); in / not_in against user.x / item.x and PG_COND_RHS_USER_LIST
 *             (list-valued properties); a bool below a bool; a domain other than item / user (:533-535); more rules, operators,
 *             list values, referenced columns or user slots than the limits; in a boost rule set an item term or item.x named
 *             `score` (the reference's clone gains a score key in the middle of the walk, boost_score_sort.go:81) and an
 *             expression over PG_COND_MAX_EXPR_OPS operations or PG_COND_MAX_EXPR_DEPTH stack slots.  PG_ERR_INVALID: unknown
 *             enum values, a name that is not declared, a boost rule without an expression (a nil dereference in the
 *             reference when its condition matches, :22-29,:82), an expression in a set that is not a boost set.
 *   Boost     (boost = 1) every rule carries a govaluate expression (pg_expr_compile_govaluate's subset) over `score` — the
 *             entry's current fp64 score — and declared columns as float64.  Per candidate, rules in order; on a match the
 *             expression's value replaces the score; without filter_all the walk ends at the first match, with it later rules
 *             see the rewritten score.  An expression that errors — a column variable of a candidate outside the store —
 *             leaves the score and still is the match (the break at :95-97 is outside the else).  out_rule: the last rule that
 *             matched, 0xFF for none.  Padding entries keep their score bits and get 0xFF.
 *   host      pg_cond_match_host / pg_boost_scores_host: pure host functions (no context, no device), the same answer stated
 *             item by item over candidate-aligned arrays: cols[d] = the n values of declared column d in its dtype (NULL for
 *             columns nothing references), item_in[i] = 0 for a candidate outside the store (NULL: all inside), user_vals
 *             [n slots] / user_present for the one request.  They validate configs and are what tests compare the kernels
 *             with; the library falls back to them for nothing.
 *   filter    pg_item_state_filter_dev evaluates rule 0 and compacts in ONE launch on the context's stream, no synchronisation
 *             (the first device call with a set uploads its lists and programs once, synchronously).  In: pg_fanin_merge_dev's
 *             outputs as they are, nq <= 256, cap <= PG_TRIM_MAX_CAP: d_rows uint64 [nq][cap], d_score fp64, optional d_source
 *             uint8, d_count [nq], d_source_mask uint32 and up to PG_TRIM_MAX_PLANES fp64 and fp32 planes [n][nq][cap]; an entry
 *             is padding if its row is UINT64_MAX or its position is >= d_count[q]: dropped, never counted.  d_user_vals
 *             [nq][PG_COND_MAX_SLOTS] 8-byte values, d_user_present [nq] bit s = slot s present (both may be NULL when the set
 *             has no user slots).  Out [nq][cap]: the kept entries in order with everything carried, d_out_count[q], and
 *             padding behind the count: UINT64_MAX rows, NaN scores and fp64 planes, source 0xFF, mask 0, fp32 planes 0 —
 *             accepted by pg_candidates_trim_dev unchanged.  Every output element is written exactly once; an output that
 *             overlaps its input is PG_ERR_INVALID.
 *   boost     pg_boost_scores_dev: d_out_score [nq][cap] and optionally d_out_rule [nq][cap] uint8; order untouched
 *             (pg_sort_scores_dev runs next); one launch, no synchronisation.  d_out_score may be d_score itself (a lane reads
 *             its entry, then writes it); any other overlap of the two is undefined.  A score an expression rewrites to NaN is
 *             "a NaN": the sign and payload of a generated or propagated NaN are the platform's (x86 and gfx950 differ); a
 *             score no rule rewrote keeps its bits, NaN payloads included.
 *   Sharing   a compiled set may be used by several contexts of ONE device, also concurrently (the upload of its table is
 *             guarded inside the set); a second device is PG_ERR_INVALID.  pg_cond_free waits for that device.
 *   one       host arrays of one request (upload, run, download, synchronise).  pg_item_state_filter: rows / score / source of
 *             the request against a store.  pg_boost_scores: pg_boost_scores_host's arguments — the candidates' own values,
 *             as a sort holds them in its items' properties — which become a store of n rows in context scratch.  n = 0 is an empty
 *             answer (PG_OK, count 0), not an error.
 *   Kernels   one lane per candidate: its row, then every referenced column's raw value — all loads issued before the first
 *             use — then the term list, a by-value kernel argument; lists and programs are read at wave-uniform addresses;
 *             the expression stack is 8 registers deep.  The filter: one workgroup of 1 024 lanes per request walks cap in
 *             chunks, wave ballots + per-wave counts in LDS give each kept entry its slot. */
#define PG_COND_MAX_RULES 8
#define PG_COND_MAX_TERMS 8
#define PG_COND_MAX_COLS 16
#define PG_COND_MAX_SLOTS 8
#define PG_COND_MAX_LIST 64
#define PG_COND_MAX_EXPR_OPS 64
#define PG_COND_MAX_EXPR_DEPTH 8
typedef enum {
    PG_COND_EQUAL = 0, PG_COND_NOT_EQUAL = 1, PG_COND_GREATER = 2, PG_COND_GREATER_THAN = 3, PG_COND_LESS = 4, PG_COND_LESS_THAN = 5,
    PG_COND_IN = 6, PG_COND_NOT_IN = 7, PG_COND_IS_NULL = 8, PG_COND_IS_NOT_NULL = 9, PG_COND_BOOL = 10,
    PG_COND_CONTAINS = 11, PG_COND_NOT_CONTAINS = 12, PG_COND_EXPRESSION = 13      /* the last three: refused by name */
} pg_cond_op;      /* "greater" is >, "greaterThan" is >=, "less" is <, "lessThan" is <= (filter_op.go:627, :801, :975, :1149) */
typedef enum { PG_COND_INT = 0, PG_COND_INT64 = 1, PG_COND_FLOAT = 2, PG_COND_STRING = 3 } pg_cond_type;
typedef enum { PG_COND_RHS_CONST = 0, PG_COND_RHS_USER = 1, PG_COND_RHS_ITEM = 2, PG_COND_RHS_USER_LIST = 3 /* refused */ } pg_cond_rhs;
typedef struct {
    const char*      name;      /* the left property (unused for PG_COND_BOOL) */
    const char*      domain;    /* "item", "user"; NULL or "" = item */
    int32_t          op;        /* pg_cond_op */
    int32_t          type;      /* pg_cond_type (ignored by is_null / is_not_null / bool) */
    int32_t          rhs;       /* pg_cond_rhs */
    uint32_t         depth;     /* 0, or 1 for a child of the bool in front */
    uint32_t         bool_and;  /* PG_COND_BOOL: 0 = or, else and */
    uint32_t         n_list;    /* in / not_in */
    long long        i;         /* the constant of int / int64 / string terms */
    double           f;         /* the constant of float terms */
    const char*      rhs_name;  /* PG_COND_RHS_USER / _ITEM: the name behind "user." / "item." */
    const long long* list;      /* in / not_in: n_list values */
} pg_cond_term;
typedef struct {
    const pg_cond_term* terms;
    uint32_t            n_terms;
    const char*         expression;   /* boost rule sets: BoostScoreCondition.Expression; else NULL */
} pg_cond_rule;
typedef struct {
    const char* name;
    int32_t     dtype;                /* pg_feature_dtype */
} pg_cond_col;
typedef struct pg_cond pg_cond;
int pg_cond_compile(const pg_cond_rule* rules, uint32_t n_rules, const pg_cond_col* cols, uint32_t n_cols, uint32_t boost, pg_cond** out);
int pg_cond_free(pg_cond* c);
int pg_cond_num_rules(const pg_cond* c);
int pg_cond_num_user_slots(const pg_cond* c);
const char* pg_cond_user_slot_name(const pg_cond* c, int i);
int pg_cond_user_slot_is_float(const pg_cond* c, int i);
int pg_cond_match_host(const pg_cond* c, uint32_t rule, uint32_t n, const uint8_t* item_in, const void* const* cols, const uint64_t* user_vals,
                       uint32_t user_present, uint8_t* out_match);
int pg_boost_scores_host(const pg_cond* c, uint32_t filter_all, uint32_t n, const uint8_t* item_in, const void* const* cols,
                         const uint64_t* user_vals, uint32_t user_present, const double* score, double* out_score, uint8_t* out_rule);
int pg_item_state_filter_dev(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                             const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                             uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32,
                             const uint64_t* d_user_vals, const uint32_t* d_user_present, uint64_t* d_out_rows, double* d_out_score,
                             uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask, float* d_out_planes_f32,
                             uint32_t* d_out_count);
int pg_boost_scores_dev(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t filter_all, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const double* d_score, const uint32_t* d_count, const uint64_t* d_user_vals, const uint32_t* d_user_present,
                        double* d_out_score, uint8_t* d_out_rule);
int pg_item_state_filter(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t n, const uint64_t* rows, const double* score,
                         const uint8_t* source, const uint64_t* user_vals, uint32_t user_present, uint64_t* out_rows, double* out_score,
                         uint8_t* out_source, uint32_t* out_count);
int pg_boost_scores(pg_ctx* ctx, pg_cond* c, uint32_t filter_all, uint32_t n, const uint8_t* item_in, const void* const* cols,
                    const uint64_t* user_vals, uint32_t user_present, const double* score, double* out_score, uint8_t* out_rule);

/* DistinctIdSort on the device (csrc/cond.hip): sort/distinct_id_sort.go:52-72 tags every item with a group id —
 * the DistinctId of the first DistinctIdCondition whose FilterParam matches, else the item's 1-based position (:57) — under one
 * property name; a later stage (DiversityRuleSort, SSD) reads it as a dimension.  A compiled condition set (not a boost set)
 * holds the conditions as its rules, in order.
 *   answer    out_id[q][p] = ids[r] for the first rule r that matches (EvaluateByDomain answers false where it errors, and
 *             :60 takes err != nil for a non-match), else p + 1; p is the position in the list as given, padding included (a
 *             list that has been through a filter has none in front of its count).  Padding entries — row UINT64_MAX or
 *             position >= d_count[q] — get 0.
 *   dev       pg_distinct_ids_dev: ids is a HOST array of pg_cond_num_rules(c) int64 (it travels as a kernel argument);
 *             d_rows uint64 [nq][cap], d_count [nq] or NULL, d_user_vals / d_user_present as pg_item_state_filter_dev,
 *             d_out_id int64 [nq][cap].  nq <= 256, cap <= PG_TRIM_MAX_CAP.  One launch, one lane per candidate, on the context's
 *             stream, no synchronisation.
 *   host      pg_distinct_ids_host: a pure host function over candidate-aligned arrays in the shape of pg_boost_scores_host;
 *             candidate i is position i of one request and none is padding.  What tests compare the kernel with; the
 *             library falls back to it for nothing.
 *   one       pg_distinct_ids: pg_distinct_ids_host's arguments through the device (the candidates' own values become a store
 *             of n rows in context scratch, as pg_boost_scores does).  n = 0 is PG_OK. */
int pg_distinct_ids_host(const pg_cond* c, const int64_t* ids, uint32_t n, const uint8_t* item_in, const void* const* cols,
                         const uint64_t* user_vals, uint32_t user_present, int64_t* out_id);
int pg_distinct_ids_dev(pg_ctx* ctx, pg_cond* c, const pg_features* fs, const int64_t* ids, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const uint32_t* d_count, const uint64_t* d_user_vals, const uint32_t* d_user_present, int64_t* d_out_id);
int pg_distinct_ids(pg_ctx* ctx, pg_cond* c, const int64_t* ids, uint32_t n, const uint8_t* item_in, const void* const* cols,
                    const uint64_t* user_vals, uint32_t user_present, int64_t* out_id);

/* The value cap on the device: DimensionFieldUniqueFilter and one dimension of GroupWeightCountFilter's size limit (DESIGN.md
 * 4.1u; csrc/dimcap.hip).  DimensionFieldUniqueFilter (filter/dimension_field_unique_filter.go:33-55) keeps the first item of each
 * value of a property — one video per author, one SKU per spu — and every item whose property is "" (:41-42);
 * groupWeightDimensionFilter (filter/group_weight_count_filter.go:288-302) keeps the first sizeLimit items of each value of a
 * dimension, "" standing for the value "__DEFAULT__" (:293-295).
 *   walk      per request, the real entries in order; padding — row UINT64_MAX or position >= min(d_count[q], cap) — is dropped
 *             and never counted.
 *   key       the value of feature-store column conf->column at the entry's row, widened to int64.  PG_F_I32 and PG_F_I64
 *             columns are served (strings are dictionary ids the caller encoded); a float column is PG_ERR_UNSUPPORTED; a name
 *             the store does not hold is PG_ERR_INVALID.
 *   null      an entry whose row is outside the store (row >= the store's rows), or, with has_null set, whose value equals
 *             null_value: the "" StringProperty returns.  PG_DIMCAP_NULL_KEEP: always kept, never counted (:41-42).
 *             PG_DIMCAP_NULL_VALUE: one more value of its own, capped like the rest ("__DEFAULT__").
 *   keep      a non-null entry is kept iff fewer than `limit` earlier entries of its key were kept in this request — that is,
 *             iff it is among the first `limit` occurrences of its key.  limit = 1 is DimensionFieldUniqueFilter exactly;
 *             limit > 1 the size limit of one dimension.  Several dimensions are several calls in the caller's order (Go
 *             walks them in map order: every order is one of its answers).  limit = 0 is PG_ERR_INVALID.
 *   dev       pg_candidates_dimcap_dev: ONE launch on the context's stream, no synchronisation.  In: the lists as
 *             pg_candidates_trim_dev takes them (pg_fanin_merge_dev's outputs as they are), nq <= 256, cap in
 *             [1, PG_TRIM_MAX_CAP], up to PG_TRIM_MAX_PLANES planes a set.  Out [nq][cap]: the kept entries in order with
 *             everything carried, d_out_count[q], and padding behind the count as pg_item_state_filter_dev pads: UINT64_MAX
 *             rows, quiet-NaN scores and fp64 planes, source 0xFF, mask 0, fp32 planes 0 — accepted by pg_candidates_trim_dev
 *             unchanged.  Every output element is written exactly once; an output that overlaps its input is PG_ERR_INVALID
 *             (the kernel reads a request's inputs after its first output is written).  Checks, in this order: the NULL
 *             arguments, the conf, nq, cap, the optional arrays' pairing, the overlap, then the column.
 *   host      pg_candidates_dimcap_host: a pure host function (no context, no device; conf->column is not read) over
 *             candidate-aligned arrays: keys int64 [nq * cap] the entries' values, item_in [nq * cap] 0 = the row is outside
 *             the store (NULL: all inside).  The statement the kernel is tested against; the library falls back to it for
 *             nothing.
 *   one       pg_candidates_dimcap: rows / score / source of one request on host arrays against a store (upload, run,
 *             download, synchronise).  n = 0 is PG_OK with count 0.
 *   Kernel    one workgroup of PG_DIMCAP_CHUNK lanes per request walks cap in chunks.  A lane loads its row, then its value;
 *             finds or claims the value's slot in an open-addressed table of full 64-bit keys with a kept-count per slot,
 *             max(2 cap, PG_DIMCAP_MIN_SLOTS) slots, linear probing from
 *                 ((uint64(key) * 0x9E3779B97F4A7C15 >> 32) * slots) >> 32;
 *             ranks itself among the lanes of its wave that hold the same slot (one ballot per bit of the slot index); then
 *             the waves take turns: count + rank < limit keeps, the last lane of a group stores min(count + group, limit).
 *             Kept entries are compacted by ballot rank and a running base.  No atomic decides an order.  Up to
 *             PG_DIMCAP_LDS_MAX_CAP the table is LDS (12 bytes a slot: 144 KiB at the boundary), above it context scratch. */
#define PG_DIMCAP_CHUNK 1024
#define PG_DIMCAP_MIN_SLOTS 1024
#define PG_DIMCAP_LDS_MAX_CAP 6144
typedef enum { PG_DIMCAP_NULL_KEEP = 0, PG_DIMCAP_NULL_VALUE = 1 } pg_dimcap_null_mode;
typedef struct {
    const char* column;        /* the feature-store column the key is read from (unused by the host statement) */
    uint32_t    limit;         /* >= 1 */
    uint32_t    null_mode;     /* pg_dimcap_null_mode */
    uint32_t    has_null;      /* != 0: a value equal to null_value is null */
    int64_t     null_value;
} pg_dimcap_conf;
int pg_candidates_dimcap_host(const pg_dimcap_conf* conf, uint32_t nq, uint32_t cap, const int64_t* keys, const uint8_t* item_in,
                              const uint64_t* rows, const double* score, const uint8_t* source, const uint32_t* count,
                              const double* planes_f64, uint32_t n_f64, const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32,
                              uint64_t* out_rows, double* out_score, uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask,
                              float* out_planes_f32, uint32_t* out_count);
int pg_candidates_dimcap_dev(pg_ctx* ctx, const pg_features* fs, const pg_dimcap_conf* conf, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                             const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                             uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                             double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                             float* d_out_planes_f32, uint32_t* d_out_count);
int pg_candidates_dimcap(pg_ctx* ctx, const pg_features* fs, const pg_dimcap_conf* conf, uint32_t n, const uint64_t* rows, const double* score,
                         const uint8_t* source, uint64_t* out_rows, double* out_score, uint8_t* out_source, uint32_t* out_count);

/* User2ItemExposureBloomFilter on the device (csrc/bloom.hip, csrc/bloom_host.hpp).  The reference keeps one Bloom
 * bitset per user in Redis (filter/user_item_exposure_bloom_filter.go; filter/bloomfilter/bloom.go, redis_bitset.go): Exists runs
 * over the candidates before rank and drops the ones it finds (user_item_exposure_bloom_filter.go:92-98), Add (logHistory) runs
 * over the returned page after the request.  Here a user's bitset is a slot of m bits in HBM, whatever the length of the history.
 *   Hash      bloom.go:67-96 hashes a value to k locations through the user's HashFunc; the one it shows is bloom_test.go:13-29:
 *             location j of key bytes d = murmur3_x86_32(d, seed_j) % m (spaolacci/murmur3 New32WithSeed), the seeds the primes
 *             of bloom_test.go:14.  That hash is served, with configurable seeds.
 *   Test      Exists is true when all k bits are set (redis_bitset.go:46-108); Set sets the k bits (redis_bitset.go:31-44).
 *   Bits      bit N of a slot is Redis's bit N: byte N >> 3, mask 0x80 >> (N & 7).  pg_bloom_slot_write takes the raw value of a
 *             user's Redis key as it is, pg_bloom_slot_read returns what can be written back.
 *   estimate  pg_bloom_estimate restates EstimateParameters (bloom.go:40-45): m = ceil(n ln p / ln(1 / 2^ln 2)), k = uint(ln 2 m / n
 *             + 0.5); PG_ERR_INVALID for n = 0 or p outside (0, 1).  A host function.
 *   keys      pg_bloom_keys holds the bytes each item-table row is hashed by — what the user's GenerateFilterValue returns,
 *             normally the item id string: offsets uint64 [rows + 1] into bytes.  Validated on the host, uploaded once: NULL
 *             arguments and offsets that descend are PG_ERR_INVALID, a key longer than PG_BLOOM_MAX_KEY bytes PG_ERR_UNSUPPORTED.
 *             A zero-length key is a key and hashes as murmur of nothing.  pg_bloom_keys_create_decimal builds the decimal text
 *             of each id (strconv.Itoa, bloom_test.go:49-51) and goes through the same upload.
 *   filter    pg_bloom_create: 1 <= m <= 2^32 - 1, 1 <= k <= PG_BLOOM_MAX_K (else PG_ERR_INVALID); seeds [k], NULL = the first k
 *             primes; n_slots >= 1 bitsets of m bits at a 256-byte-aligned stride (pg_bloom_info's bytes per slot), zeroed.  The
 *             mapping from a user to a slot is the host's, as the Redis key is in the reference.
 *   slots     pg_bloom_slot_write: n <= ceil(m / 8) Redis-order bytes, the rest of the slot zeroed; bits at or above m in the last
 *             byte are ignored and read back as 0.  pg_bloom_slot_read: n <= ceil(m / 8) bytes.  pg_bloom_slot_clear.  All three
 *             synchronise; a slot >= n_slots or an n above ceil(m / 8) is PG_ERR_INVALID.
 *   device    pg_bloom_exists_dev / pg_bloom_filter_dev / pg_bloom_add_dev: enqueued on the context's stream, no synchronisation,
 *             nq <= 256, cap <= PG_TRIM_MAX_CAP.  d_slots [nq]: the slot of each request, PG_BLOOM_NO_SLOT = a user without
 *             history; a slot >= n_slots is treated as PG_BLOOM_NO_SLOT and reads or writes nothing.  A padding entry (row
 *             UINT64_MAX, or a position at or behind d_count[q]) is never kept and never added.  A row outside the key store has
 *             no key: its Exists is false, so it is kept, and Add skips it.
 *               exists   d_out_exists uint8 [nq][cap]: 1 where all k bits are set; padding positions 0.
 *               filter   pg_item_state_filter_dev's argument list with b, keys, d_slots in place of the condition set, the feature
 *                        store and the user values, its checks in its order, its outputs: the entries whose Exists is false, in
 *                        order, with everything carried, d_out_count[q], padding behind the count as that stage pads.  With
 *                        PG_BLOOM_NO_SLOT the real entries come out bit for bit as they went in.  Two launches.
 *               add      sets the k bits of every real entry in its request's slot (atomic ORs on 32-bit words: two requests
 *                        of one call may name one slot).  Stream order is the only fence: an add followed by a filter on the
 *                        same stream sees the added bits.
 *   one       pg_bloom_filter / pg_bloom_add / pg_bloom_exists: one request on host arrays (upload, run, download, synchronise);
 *             n = 0 is an empty answer.
 *   host      pg_bloom_*_host: the same answers over host arrays — bitsets [n_slots][ceil(m / 8)] Redis bytes, the keys as
 *             offsets + bytes — with the same checks; no context, no device.  pg_bloom_murmur3_host is the hash itself.  They are
 *             what tests compare the kernels with; the library falls back to them for nothing.
 *   Kernels   probe: one lane per candidate, grid (cap / 256, nq); the lane loads its key, mixes each 4-byte block once for all
 *             seeds, folds and finalises per seed, issues its k word loads together and writes one keep ballot per wave into
 *             context scratch.  compaction: one workgroup per request walks the ballots (block_rank.hpp, cand_carry, cand_pad).
 *             add: the probe's grid and arithmetic, then atomic ORs.
 *   Not here  RedisBloomFilter (BF.MADD, RedisBloom's own hash); rotation (bloom_rotation.go: a host that rotates holds several
 *             pg_bloom objects, adds to all and tests the active one); keys longer than PG_BLOOM_MAX_KEY bytes. */
#define PG_BLOOM_MAX_KEY 64
#define PG_BLOOM_MAX_K 16
#define PG_BLOOM_NO_SLOT 0xFFFFFFFFu
typedef struct pg_bloom pg_bloom;
typedef struct pg_bloom_keys pg_bloom_keys;
int pg_bloom_estimate(uint64_t n, double p, uint64_t* m, uint32_t* k);
int pg_bloom_murmur3_host(const uint8_t* bytes, uint64_t n, uint32_t seed, uint32_t* out);
int pg_bloom_keys_create(pg_ctx* ctx, uint64_t rows, const uint64_t* offsets, const uint8_t* bytes, pg_bloom_keys** out);
int pg_bloom_keys_create_decimal(pg_ctx* ctx, uint64_t rows, const int64_t* ids, pg_bloom_keys** out);
int pg_bloom_keys_free(pg_ctx* ctx, pg_bloom_keys* keys);
int pg_bloom_create(pg_ctx* ctx, uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, pg_bloom** out);
int pg_bloom_free(pg_ctx* ctx, pg_bloom* b);
int pg_bloom_info(const pg_bloom* b, uint64_t* m, uint32_t* k, uint32_t* n_slots, uint64_t* slot_bytes);
int pg_bloom_slot_write(pg_ctx* ctx, pg_bloom* b, uint32_t slot, const uint8_t* bytes, uint64_t n);
int pg_bloom_slot_read(pg_ctx* ctx, const pg_bloom* b, uint32_t slot, uint8_t* bytes, uint64_t n);
int pg_bloom_slot_clear(pg_ctx* ctx, pg_bloom* b, uint32_t slot);
int pg_bloom_exists_dev(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const uint32_t* d_count, const uint32_t* d_slots, uint8_t* d_out_exists);
int pg_bloom_filter_dev(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64, uint32_t n_f64,
                        const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, const uint32_t* d_slots,
                        uint64_t* d_out_rows, double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64,
                        uint32_t* d_out_source_mask, float* d_out_planes_f32, uint32_t* d_out_count);
int pg_bloom_add_dev(pg_ctx* ctx, pg_bloom* b, const pg_bloom_keys* keys, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                     const uint32_t* d_count, const uint32_t* d_slots);
int pg_bloom_exists(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t n, const uint64_t* rows, uint32_t slot,
                    uint8_t* out_exists);
int pg_bloom_filter(pg_ctx* ctx, const pg_bloom* b, const pg_bloom_keys* keys, uint32_t n, const uint64_t* rows, const double* score,
                    const uint8_t* source, uint32_t slot, uint64_t* out_rows, double* out_score, uint8_t* out_source, uint32_t* out_count);
int pg_bloom_add(pg_ctx* ctx, pg_bloom* b, const pg_bloom_keys* keys, uint32_t n, const uint64_t* rows, uint32_t slot);
int pg_bloom_exists_host(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, const uint8_t* bitsets, uint64_t key_rows,
                         const uint64_t* key_offsets, const uint8_t* key_bytes, uint32_t nq, uint32_t cap, const uint64_t* rows,
                         const uint32_t* count, const uint32_t* slots, uint8_t* out_exists);
int pg_bloom_add_host(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, uint8_t* bitsets, uint64_t key_rows,
                      const uint64_t* key_offsets, const uint8_t* key_bytes, uint32_t nq, uint32_t cap, const uint64_t* rows,
                      const uint32_t* count, const uint32_t* slots);
int pg_bloom_filter_host(uint64_t m, uint32_t k, const uint32_t* seeds, uint32_t n_slots, const uint8_t* bitsets, uint64_t key_rows,
                         const uint64_t* key_offsets, const uint8_t* key_bytes, uint32_t nq, uint32_t cap, const uint64_t* rows,
                         const double* score, const uint8_t* source, const uint32_t* count, const double* planes_f64, uint32_t n_f64,
                         const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32, const uint32_t* slots, uint64_t* out_rows,
                         double* out_score, uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask, float* out_planes_f32,
                         uint32_t* out_count);
int pg_bloom_slot_write_host(uint64_t m, uint32_t n_slots, uint8_t* bitsets, uint32_t slot, const uint8_t* bytes, uint64_t n);

/* DiversityAdjustCountFilter on the device: quotas per expression class (csrc/classcut.hip).  The fourth reference
 * filter of the slot between UniqueFilter and RankService.Rank (service/user_recommend.go:105-137): every AdjustCountConfig gives
 * its quota not to a recall but to the items for which a govaluate expression over the item's features is true
 * (filter/diversity_adjust_count_filter.go:75-143), e.g. recall_name == 'u2i' && category == 3.  Classes may overlap; an item an
 * earlier class took is skipped by later ones.
 *   In        pg_fanin_merge_dev's outputs as they are, in pg_candidates_trim_dev's argument order and optionality (nq <= 256, cap
 *             in [1, PG_TRIM_MAX_CAP]), + the compiled set and the pg_features store its columns are bound to by name (NULL only for a set that reads no
 *             column).  An entry
 *             is padding if its row is UINT64_MAX or its position is >= d_count[q]; padding may sit anywhere, is dropped and
 *             never counted.
 *   Answer    DEFINED bit for bit (doFilter, :75-143; only the order among equal scores is being fixed, as for the trim):
 *               1. a request's real entries are put in pg_sort_scores_dev's order of d_score: descending, -0.0 equals +0.0,
 *                  NaN last, ties keep input position (the reference shuffles the first half and sorts unstably, :83-87);
 *               2. class c (rule c, c < n <= PG_CLASSCUT_MAX_CLASSES) holds, in that order, the entries for which expression c
 *                  evaluates to true (:92-103: an evaluation error or any other result is "not a member");
 *               3. classes apply in rule order with acc = 0 (:115-140): limit_c = count_c for PG_TRIM_FIX, max(0, count_c -
 *                  acc) for PG_TRIM_ACCUMULATE; the window of class c is its first limit_c members (the reference's `i < count`
 *                  indexes the class's list: a member an earlier class took still uses up a place); its picks are the window's
 *                  members no earlier class picked, in order; an ACCUMULATE class then adds its picks to acc;
 *               4. the output is the picks concatenated in class order, then the trim's padding: row UINT64_MAX, score -inf,
 *                  source 0xFF, fp64 planes 0x7FF8000000000000, mask 0, fp32 planes 0; d_out_count[q] = the number of picks.
 *             Every carried array is gathered through the same permutation; score and source are unchanged; no value meets
 *             arithmetic, doubles and floats travel as bits.  Outputs are [nq][out_cap] with out_cap from pg_classcut_out_cap;
 *             an output is required exactly where its input is given; an output that overlaps its input is PG_ERR_INVALID.
 *   Language  govaluate at the version the reference pins (go.mod: v3.0.1-0.20171022003610), as a STATICALLY TYPED boolean subset
 *             compiled to the postfix program of pg_expr_compile_govaluate (parity is unpinned: the library is Go).
 *             Numbers: everything pg_expr_compile_govaluate accepts — float64 literals, bare and [bracketed] names, + - * / % **,
 *             unary minus, parentheses, round — with its precedence.  Comparators == != > >= < <= on two numbers, IEEE (NaN ==
 *             x false, NaN != x true), looser than arithmetic; x in (a, b, …) over 2 .. PG_COND_MAX_LIST constant numbers,
 *             tested by ==; && looser than the comparators, || looser still, both left-associative; prefix ! on a bool.
 *             Variables: DECLARED item columns {name, dtype}, bound by name to the store at run time as pg_cond binds them and
 *             read as float64(value) (only referenced columns are loaded; dictionary-coded strings compare as their codes);
 *             recall_score = the entry's d_score (module/item.go:229-248); recall_name = the entry's source as a string through
 *             recall_names[n_recalls] (n_recalls <= PG_CLASSCUT_MAX_RECALLS), legal only as recall_name == 'lit', != 'lit' and
 *             in ('a', 'b', …) with ' or " quotes and literals of the shape [A-Za-z_][A-Za-z0-9_]* (govaluate tries every string
 *             as a date first; this shape never is one); a literal that names no recall equals nothing, a source >= n_recalls
 *             has a name equal to no literal.
 *   Errors    a candidate whose row is >= the store's rows has every declared column missing (recall_name and recall_score are
 *             still there); reading one is govaluate's "No parameter found".  An error propagates through arithmetic,
 *             comparators, in and !; a && b is a's error, false if a is false (b is not looked at), else b; a || b the same with
 *             true; a final error means "not a member" (:95-98).
 *   Refused   by name at compile, nothing allocated.  PG_ERR_UNSUPPORTED: the ternary and ??; bitwise operators, =~ and !~; true /
 *             false; == / != between bools; ordered comparisons on, or arithmetic with, recall_name; any other string literal; a
 *             top-level expression that is a number; a bool where a number is needed or a number where a bool is (errors on every
 *             item in govaluate); a one-element in list; every other function, accessors, a chained **; more than
 *             PG_COND_MAX_EXPR_OPS operations, PG_COND_MAX_EXPR_DEPTH stack slots, PG_COND_MAX_COLS referenced columns or 4096
 *             in-list values per set; more than PG_CLASSCUT_MAX_CLASSES classes; anything malformed.  PG_ERR_INVALID: no classes
 *             (the reference indexes configs[len - 1], :115); an ACCUMULATE class directly after an ACCUMULATE class with a larger
 *             count (the reference panics in its constructor, :56-61); a type other than FIX / ACCUMULATE; a name that is neither
 *             declared nor a built-in (that includes the reference's per-recall Properties key).  At a call, on the host and with
 *             the context left usable: an expression that reads recall_name while d_source is absent (PG_ERR_INVALID); cap outside
 *             [1, PG_TRIM_MAX_CAP] (PG_ERR_UNSUPPORTED).
 *   Width     pg_classcut_out_cap: a pure host function; out_cap = min(cap, the sum of the FIX counts + the largest ACCUMULATE
 *             count) — no request keeps more.
 *   host      pg_classcut_masks_host (n candidates → one byte each, bit c = member of class c) and pg_candidates_classcut_host
 *             (the whole answer): pure host functions over candidate-aligned arrays as pg_cond_match_host takes them — cols[d] =
 *             the values of declared column d in its dtype (NULL for columns nothing references), item_in[i] = 0 for a candidate
 *             outside the store (NULL: all inside); for the whole answer both are [nq * cap].  The statements the kernels are
 *             tested against; the library falls back to them for nothing.
 *   Kernels   pg_classcut_masks_dev: ONE launch, one lane per candidate — its row, every referenced column's raw value (all loads
 *             issued before the first use), then each class's program on an 8-deep register stack with one error bit beside each
 *             slot; programs and lists are read at wave-uniform addresses; every byte of [nq][cap] is written, padding gets 0.
 *             pg_candidates_classcut_dev: that launch, the trim's score sort, and one workgroup of PG_TRIM_CHUNK lanes per
 *             request: classes one after another, each walking the sorted order PG_TRIM_CHUNK positions at a time (a member's
 *             rank from wave ballots, per-wave counts in LDS and the running count; picked iff in the window and its bit in a
 *             2 KB LDS bitmap of input positions is clear) up to the chunk in which the rank reaches the limit; then the padding.
 *             Every output element is written exactly once.
 *   Stream    the device calls enqueue on the context's stream and do not synchronise (the first device call with a set uploads
 *             its lists and programs once, synchronously).  Sharing and free: as pg_cond — several contexts of ONE device may
 *             use a set, also concurrently; pg_classcut_free waits for that device.
 *   one       pg_candidates_classcut: one request on host arrays against a store (upload, run, download, synchronise), outputs
 *             [pg_classcut_out_cap(n)]; n = 0 is an empty answer. */
#define PG_CLASSCUT_MAX_CLASSES 8
#define PG_CLASSCUT_MAX_RECALLS 32
typedef struct {
    const char* expression;   /* AdjustCountConfig.Expression */
    uint8_t     type;         /* PG_TRIM_FIX | PG_TRIM_ACCUMULATE (AdjustCountConfig.Type "fix" / "accumulator") */
    uint32_t    count;
} pg_classcut_rule;
typedef struct pg_classcut pg_classcut;
int pg_classcut_compile(const pg_classcut_rule* rules, uint32_t n, const pg_cond_col* cols, uint32_t n_cols, const char* const* recall_names,
                        uint32_t n_recalls, pg_classcut** out);
int pg_classcut_free(pg_classcut* c);
int pg_classcut_num_classes(const pg_classcut* c);
int pg_classcut_reads_recall_name(const pg_classcut* c);
int pg_classcut_out_cap(const pg_classcut* c, uint32_t cap, uint32_t* out_cap);
int pg_classcut_masks_host(const pg_classcut* c, uint32_t n, const uint8_t* item_in, const void* const* cols, const uint8_t* source,
                           const double* score, uint8_t* out_masks);
int pg_candidates_classcut_host(const pg_classcut* c, uint32_t nq, uint32_t cap, const uint8_t* item_in, const void* const* cols,
                                const uint64_t* rows, const double* score, const uint8_t* source, const uint32_t* count,
                                const double* planes_f64, uint32_t n_f64, const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32,
                                uint64_t* out_rows, double* out_score, uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask,
                                float* out_planes_f32, uint32_t* out_count);
int pg_classcut_masks_dev(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                          const double* d_score, const uint8_t* d_source, const uint32_t* d_count, uint8_t* d_out_masks);
int pg_candidates_classcut_dev(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                               const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                               uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                               double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                               float* d_out_planes_f32, uint32_t* d_out_count);
int pg_candidates_classcut(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t n, const uint64_t* rows, const double* score,
                           const uint8_t* source, uint64_t* out_rows, double* out_score, uint8_t* out_source, uint32_t* out_count);

/* MultiRecallMixSort on the device: fixed and random page slots (csrc/mixsort.hip).  The reference's page-shaping
 * sort behind ItemRankScore (sort/multi_recall_mix_sort.go, sort/mix_sort_strategy.go): every MixSortConfig is a strategy that
 * claims items by recall name or by a module.FilterParam and puts them at configured positions of the page (fix_position) or at
 * a random place of each stride (random_position); everything else fills up in order.
 *   In        one request holds entries 0 .. n-1, n = d_count[q] (cap when d_count is NULL), in the order the previous sort left
 *             them; an entry's position in that list is its identity (after UniqueFilter ids are unique, so remainItemIterator's
 *             id map, :180-216, is a "placed" flag per entry).  d_order [nq][cap] uint32 (optional, NULL =
 *             identity): list entry j is element d_order[q][j] of the [nq][cap] arrays — pg_sort_scores_dev's output and the
 *             recommend calls' d_out_order plug in as they are.  Per element: d_rows uint64 (binds the condition columns and the
 *             position columns through a pg_features store; a row >= the store's rows is "missing", as for pg_cond), d_source
 *             uint8 (the fan-in's numbering; required iff a strategy has a non-zero source mask), user slots as pg_cond takes
 *             them (d_user_vals [nq][PG_COND_MAX_SLOTS], d_user_present [nq]).  S = max(ctx_size, the compiled size) (:42-45,
 *             :66-69); ctx_size is one host value per call; 1 <= S <= PG_MIX_MAX_SIZE.
 *   Answer    DEFINED bit for bit; positions are reported as indices into the [nq][cap] arrays (composed with d_order).
 *               1. n < S: the answer is the identity, the count n (:71-73).
 *               2. strategies s = 0 .. n_s-1 in config order.  number_s (mix_sort_strategy.go:121-176): FIX — the number of
 *                  configured positions, else `number` if > 0, else 0; RANDOM — (int)((double)S * number_rate) if number_rate >
 *                  0, else `number` if > 0, else 0.  member_s(i): the source bit of entry i is set in the strategy's mask (a
 *                  source >= 32 never matches), or the strategy has conditions and they hold (:86-107).  Inside pg_cond's subset
 *                  EvaluateByDomain returns no error, so the break at :95-98 is unreachable.
 *               3. taken_s = the first number_s entries, in list order, with member_s that no earlier strategy took; D = the first
 *                  S entries nobody took.  (The reference walks item by item, strategies inside, and stops once all are full,
 *                  :82-128; taking strategy by strategy gives the same lists.)
 *               4. result[0 .. S) starts empty.  FIX strategies first, in config order (BuildItems, :137-155): P_s = the
 *                  configured positions; or, without any and with a position column, for j < min(number_s, |taken_s|) the column's
 *                  value at taken_s[j] (a missing row counts as -1, utils.ToInt(.., -1)), keeping the values p > 0 in order.
 *                  idx = 0; for each p in P_s: if p <= S and idx < |taken_s|, result[p-1] = taken_s[idx++].  A later write to a
 *                  slot replaces the earlier entry, which then is no longer in the result.  (The k-th usable position receives
 *                  the k-th taken entry, not the entry whose column gave the position: that is the reference.)
 *               5. RANDOM strategies next, in config order (:178-216): step = S / number_s, start = 0; for the j-th entry of
 *                  taken_s: stop if no slot of result is empty; end = min(start + draw(q, s, j) % step, S - 1), moved forward
 *                  cyclically to the first empty slot; the entry goes there; start += step.
 *                  draw(q, s, j): x = seed[q] + 0x9E3779B97F4A7C15 * (1 + s * 65536 + j) in uint64 arithmetic;
 *                  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9; x = (x ^ (x >> 27)) * 0x94D049BB133111EB; draw = x ^ (x >> 31) (the
 *                  splitmix64 finaliser).  d_seed [nq] uint64, NULL = 0.  Go's process-wide math/rand stream is not reproduced;
 *                  the range and the placement rule are.
 *               6. D fills the empty slots in ascending slot order (:236-245).
 *               7. slots still empty receive, in ascending slot order, the entries not in result, in list order (:143-159).
 *                  Because n >= S there are always enough: the shrinking branch :152-156 is unreachable, |result| = S exactly,
 *                  without duplicates.
 *               8. with remain_item every entry not in the result follows in list order (:161-174) and the count is n; otherwise
 *                  the count is S.  Slots behind the count receive UINT32_MAX.  Every element of d_out_order [nq][cap] and
 *                  d_out_count [nq] is written exactly once; d_out_order may not overlap d_order.
 *   Refused   on the host, the context left usable.  PG_ERR_INVALID: a configured position < 1 (the reference indexes items[-1]);
 *             a RANDOM strategy with number_s > S at the call's S (rand.Intn(0) panics); a negative number / number_rate; a
 *             source mask without d_source; a position column that is not declared int32 / int64 or is not in the store; an
 *             unknown strategy type.  PG_ERR_UNSUPPORTED: more than PG_MIX_MAX_STRATEGIES strategies; more than
 *             PG_MIX_MAX_POSITIONS positions in one strategy; S > PG_MIX_MAX_SIZE; cap outside [1, PG_TRIM_MAX_CAP]; nq > 256;
 *             whatever pg_cond_compile refuses, under its name.  No strategies is not an error: the answer is D, then the tail.
 *   host      pg_mix_sort_host: a pure host function (no context, no device), the same answer stated entry by entry over
 *             candidate-aligned arrays as pg_candidates_classcut_host takes them: cols[d] = the nq * cap values of declared
 *             column d in its dtype (NULL for columns nothing reads), item_in[i] = 0 for an element outside the store (NULL: all
 *             inside), source, user_vals [nq][PG_COND_MAX_SLOTS], user_present [nq].  What the kernels are tested against; the
 *             library falls back to it for nothing.
 *   Kernels   pg_mix_sort_dev: two launches on the context's stream, no synchronisation (the first device call with a set
 *             uploads its position table once, synchronously).  A match kernel, one lane per entry: its row, every referenced
 *             column's raw value (all loads issued before the first use), each strategy's rule and source mask → one byte, bit s
 *             = member of strategy s.  A mix kernel, one workgroup of 1 024 lanes per request: strategies in turn walk the list
 *             1 024 entries at a time (rank from wave ballots + per-wave counts; a 2 KB LDS bitmap of taken entries; the walk
 *             ends in the chunk where the rank reaches number_s), one wave places FIX and RANDOM entries into the page in LDS,
 *             all lanes fill and write the tail from an "in result" bitmap.  No entry depends on which lane came first.
 *   Sharing   as pg_cond: several contexts of ONE device may use a set, also concurrently; pg_mix_free waits for that device.
 *   one       pg_mix_sort: one request on host arrays against a store (upload, run, download, synchronise); n = 0 is an empty
 *             answer. */
#define PG_MIX_FIX 1            /* MixStrategy "fix_position" */
#define PG_MIX_RANDOM 2         /* MixStrategy "random_position" */
#define PG_MIX_MAX_STRATEGIES 8
#define PG_MIX_MAX_POSITIONS 256
#define PG_MIX_MAX_SIZE 4096
typedef struct {
    int32_t             type;            /* PG_MIX_FIX | PG_MIX_RANDOM */
    const int32_t*      positions;       /* FIX: MixSortConfig.Positions, 1-based */
    uint32_t            n_positions;
    const char*         position_field;  /* FIX without positions: MixSortConfig.PositionField, a declared int32 / int64 column; NULL or "" = none */
    int32_t             number;          /* MixSortConfig.Number */
    double              number_rate;     /* MixSortConfig.NumberRate (RANDOM) */
    uint32_t            source_mask;     /* bit r = RecallNames holds the fan-in's source r */
    const pg_cond_term* terms;           /* MixSortConfig.Conditions */
    uint32_t            n_terms;
} pg_mix_strategy;
typedef struct pg_mix pg_mix;
int pg_mix_compile(const pg_mix_strategy* strategies, uint32_t n, const pg_cond_col* cols, uint32_t n_cols, uint32_t size, uint32_t remain_item,
                   pg_mix** out);
int pg_mix_free(pg_mix* m);
int pg_mix_num_strategies(const pg_mix* m);
int pg_mix_num_user_slots(const pg_mix* m);
const char* pg_mix_user_slot_name(const pg_mix* m, int i);
int pg_mix_user_slot_is_float(const pg_mix* m, int i);
int pg_mix_sort_host(const pg_mix* m, uint32_t ctx_size, uint32_t nq, uint32_t cap, const uint8_t* item_in, const void* const* cols,
                     const uint8_t* source, const uint32_t* order, const uint32_t* count, const uint64_t* seed, const uint64_t* user_vals,
                     const uint32_t* user_present, uint32_t* out_order, uint32_t* out_count);
int pg_mix_sort_dev(pg_ctx* ctx, pg_mix* m, const pg_features* fs, uint32_t ctx_size, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                    const uint8_t* d_source, const uint32_t* d_order, const uint32_t* d_count, const uint64_t* d_seed,
                    const uint64_t* d_user_vals, const uint32_t* d_user_present, uint32_t* d_out_order, uint32_t* d_out_count);
int pg_mix_sort(pg_ctx* ctx, pg_mix* m, const pg_features* fs, uint32_t ctx_size, uint32_t n, const uint64_t* rows, const uint8_t* source,
                const uint32_t* order, uint64_t seed, const uint64_t* user_vals, uint32_t user_present, uint32_t* out_order,
                uint32_t* out_count);

/* TrafficControlSort's macro control on the device (csrc/traffic.hip, csrc/traffic_host.hpp).  The reference's
 * sort (sort/traffic_control_sort.go) splits per request into a controller — PIDController.compute / setMeasurement,
 * computeMacroControlAlpha, filterValidControllers: a handful of scalars per target, driven by wall-clock time and remote traffic
 * counters, which stay on the host and hand over ONE number per target and request, alpha — and the re-ranking: macroControl
 * (:204-364), computeDeltaRank (:555-589) and the closing position sort (:160-181), N items x T targets, which is this stage.
 *   In        one request holds entries 0 .. n-1, n = d_count[q] (cap when d_count is NULL); d_order [nq][cap] uint32 (optional,
 *             NULL = identity): list entry j is element d_order[q][j] of the [nq][cap] arrays, as for pg_mix_sort_dev.  Per element:
 *             d_score fp64 (Item.Score), d_member uint8: bit t set = isControlledItem(controller_t, item) — the output of
 *             pg_classcut_masks_dev over a set whose class expressions are the targets' item expressions plugs in as it is (its
 *             counts are ignored; hence at most 8 targets); a target without an item expression has its bit on every entry.
 *             d_alpha [nq][T] fp64: the controller's output for that request; 0 = the target is off for this request (filtered
 *             out, returned 0, timed out).  An order value >= cap is PG_ERR_INVALID where the host can see it (the host statement
 *             and the one-request call); on the device it is padding as in pg_ssd_sort_dev: the entry leaves the list first and
 *             appears in no output.  Scalars per call: ctx_size (ctx.Size), page_no (the page_number parameter, clamped to >= 1
 *             by the caller as :294-297 does), gamma, beta, eta (PidGamma, PidBeta, PidEta: 1.0, 1.0, 1.6 by default, :269-282).
 *   Answer    DEFINED bit for bit.
 *               0. The list is taken to be score-descending already: the stage does not redo :114's unstable sort.Sort and keeps the
 *                  order that arrives (the rule and the reason of pg_ssd_sort_dev).  i is the list index, origin_i = i + 1 and
 *                  control_id_i starts at i + 1 (:115-118).
 *               1. n = 0, T = 0 or every alpha of the request 0: the identity (:131-135, :208-211), control_id_i = i + 1,
 *                  new_pos_i = i + 1.  (The steps below give exactly that; nothing is a special case.)
 *               2. goint(x): Go's float64 -> int on amd64 — truncation toward zero for -2^63 < x < 2^63, INT64_MIN for NaN and
 *                  everything else.  All integer arithmetic behind it is wrapping int64 (in sigmoid, INT64_MIN - 5000 wraps
 *                  positive and returns 1; in step 6, ctx_size + goint(NaN) is hugely negative).
 *               3. Tables (:45-66), built once with the host's libm (pg_traffic_table reads them; the device receives them by
 *                  upload and never computes them): positionWeight[i] = exp(-0.01 * i) for i < 500 and the literal 0.006737946999
 *                  beyond, expTable[i] = exp(i / 1000.0), tanhTable[i] = tanh(i / 1000.0), sigmoidTable[i] = 1 / (1 + exp(10 -
 *                  (i / 1000.0 + 5.0))).
 *               4. Scores and sums (:217-256): s_i = score_i with 0.0 replaced by 1e-8; maxScore = s_0; itemScore_0 = math.E (the
 *                  constant, not exp(1.0)), itemScore_i = expTable[clamp(goint(s_i / maxScore * 1000), 0, 999)] for i > 0;
 *                  w_i = s_i * posWeight_i; total = sum of w_i; sum_t = sum of w_i over the entries with bit t, for the targets
 *                  with alpha_t != 0.  Both run sequentially in list order from 0.0 (the reference's chains; fp64 addition is not
 *                  associative).  weight_t = sum_t / total if target t received at least one addition, else 0.0 (the map has no
 *                  key); the division as written, so it may be NaN or +-Inf.
 *               5. Uplift scaling (:284-291): for alpha_t > 0, alpha_t *= 1.0 + gamma * tanh_tab(beta * weight_t), with
 *                  tanh_tab(x) = tanhTable[clamp(goint(x * 1000), 0, 2999)] (:942-950).  Every product and sum is its own
 *                  operation (no fused multiply-add).
 *               6. Per entry i (:332-356), targets t in ascending index, final = 0.0.  (The reference walks a Go map; only the last
 *                  bit of `final` and the control id of an entry two targets uplift depend on that order.  Ascending is the
 *                  definition.)  Skip t if bit t is clear or alpha_t (as step 5 left it) == 0.
 *                    alpha_t < 0 (pull down): rho = eta * (1.0 - tanh_tab(weight_t)); delta = alpha_t * sigmoid_tab(double(i), rho);
 *                      sigmoid_tab(x, rho): idx = goint(rho * x * 1000.0) - 5000; idx < 0 uses entry 0, idx >= 10000 returns 1.0,
 *                      otherwise sigmoidTable[idx] (:952-960).
 *                    otherwise (uplift; a NaN alpha lands here, as in Go): delta = alpha_t * itemScore_i; start = ctx_size, and if
 *                      page_no > 1, start += goint((weight_t - 0.3) * 10 * double(ctx_size)); if i > start and delta >= 1.0:
 *                      PG_TRAFFIC_PERCENT sets control_id_i = -target_id, PG_TRAFFIC_QUANTITY sets it to 0 if it is > 0.
 *                    final += delta.
 *                  Behind the targets: if final != 0.0 and control_id_i == 0 and final < 1.0, control_id_i = origin_i (:350-356).
 *               7. Positions (:160-180): new_pos_i = final != 0.0 ? double(i + 1) - final : double(i + 1).  A NaN new_pos is
 *                  reported as the quiet NaN 0x7FF8000000000000 (IEEE 754 leaves a NaN's sign and payload to the hardware).
 *               8. Order (:181, ItemRankSlice :924-934): ascending new_pos (-0.0 equal to +0.0), ties by origin position; a NaN
 *                  new_pos sorts behind every number, NaNs among themselves by origin.  (The reference's comparator is no order
 *                  there: this is a definition.)  The count is n.
 *   Outputs   d_out_order [nq][cap] uint32: indices into the [nq][cap] arrays (composed with d_order), UINT32_MAX behind the count;
 *             d_out_count [nq]; optional d_out_control_id [nq][cap] int32 (__traffic_control_id__) by input element, 0 for an
 *             element that is no entry of the list; optional d_out_new_pos [nq][cap] fp64 (_NEW_POSITION_) by input element, the
 *             quiet NaN 0x7FF8000000000000 for such an element.  Every element of every output is written exactly once (d_order
 *             names no element twice).  An output that overlaps an input or another output is PG_ERR_INVALID.
 *   Refused   pg_traffic_compile, by name, nothing allocated: more than PG_TRAFFIC_MAX_TARGETS targets or an unknown control type
 *             (PG_ERR_UNSUPPORTED); target_id == INT32_MIN, whose negation overflows (PG_ERR_INVALID).  No targets compiles: the
 *             answer is the identity.  A call, on the host, the context left usable: nq = 0, ctx_size == 0, page_no == 0, a
 *             missing score / member / alpha while T > 0 (PG_ERR_INVALID); nq > 256, cap outside [1, PG_TRIM_MAX_CAP]
 *             (PG_ERR_UNSUPPORTED).
 *   host      pg_traffic_sort_host: a pure host function (no context, no device), the answer entry by entry; what the kernels are
 *             tested against, the library falls back to it for nothing.  out_control_id / out_new_pos may be NULL.
 *   Kernels   pg_traffic_sort_dev: enqueued on the context's stream, no synchronisation (the first device call with a set uploads
 *             the four tables once, synchronously).  A control kernel, one workgroup of PG_TRIM_CHUNK lanes per request: lanes walk
 *             the list a chunk at a time, compact it (wave ballots), stage w_i and the member byte in LDS; lanes 0 .. T of the
 *             first wave each run one sequential chain over the chunk (lane 0 total, lane 1 + t sum_t and its "received an
 *             addition" flag); one lane per target then finishes weight_t, the scaled alpha, rho and the page-2 start; all lanes
 *             do steps 6 and 7 from the tables in global memory (116 KB, read-only, data-dependent addresses: they stay in L2)
 *             and write new_pos and control_id by element and new_pos in list order as the sort key.  The order is the segmented
 *             score sort of pg_sort_scores_dev, ascending: its ties-keep-input-order and NaN-last rules are step 8's.  A compose
 *             kernel maps the sorted positions to elements and writes the UINT32_MAX tail and the counts.
 *   Sharing   as pg_mix: several contexts of ONE device may use a set, also concurrently; pg_traffic_free waits for that device.
 *   one       pg_traffic_sort: one request of n entries on host arrays (upload, run, download, synchronise); alpha [T]; n = 0 is an
 *             empty answer.
 *   Not here  microControl (:592-704), sampleControlTargetsByScore (:502-545), the controller and the isControlledBy* filters. */
#define PG_TRAFFIC_MAX_TARGETS 8
#define PG_TRAFFIC_PERCENT  1   /* task.ControlType "Percent" */
#define PG_TRAFFIC_QUANTITY 2   /* anything else */
typedef struct {
    int32_t target_id;          /* strconv.Atoi(TrafficControlTargetId) */
    int32_t control_type;       /* PG_TRAFFIC_PERCENT | PG_TRAFFIC_QUANTITY */
} pg_traffic_target;
typedef struct pg_traffic pg_traffic;
int pg_traffic_compile(const pg_traffic_target* targets, uint32_t n, pg_traffic** out);
int pg_traffic_free(pg_traffic* m);
int pg_traffic_num_targets(const pg_traffic* m);
/* entries [first, first + n) of table `which`: 0 positionWeight[500], 1 expTable[1000], 2 tanhTable[3000], 3 sigmoidTable[10000] */
int pg_traffic_table(int which, uint32_t first, uint32_t n, double* out);
int pg_traffic_sort_host(const pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta, uint32_t nq,
                         uint32_t cap, const double* score, const uint8_t* member, const uint32_t* order, const uint32_t* count,
                         const double* alpha, uint32_t* out_order, uint32_t* out_count, int32_t* out_control_id, double* out_new_pos);
int pg_traffic_sort_dev(pg_ctx* ctx, pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta,
                        uint32_t nq, uint32_t cap, const double* d_score, const uint8_t* d_member, const uint32_t* d_order,
                        const uint32_t* d_count, const double* d_alpha, uint32_t* d_out_order, uint32_t* d_out_count,
                        int32_t* d_out_control_id, double* d_out_new_pos);
int pg_traffic_sort(pg_ctx* ctx, pg_traffic* m, uint32_t ctx_size, uint32_t page_no, double gamma, double beta, double eta, uint32_t n,
                    const double* score, const uint8_t* member, const uint32_t* order, const double* alpha, uint32_t* out_order,
                    uint32_t* out_count, int32_t* out_control_id, double* out_new_pos);

/* SSDSort on the device: candidate lists in, re-ranked page out (csrc/ssd.hip).  SSDSort.Sort and doSort around the
 * sliding window (sort/ssd_sort.go:110-343) for nq requests on device arrays: the ssd_filter_retrieve_ids split, the candidate-count
 * cut, the min-score-percent cut, the two normalisations with their "all item score are zeros" bail-out, SSDWithSlidingWindow
 * (:346-486, as pg_ssd) and the backup list behind the picks.  Enqueued on the context's stream; no host synchronisation.
 *   In        one request holds entries 0 .. n-1, n = d_count[q] (cap when d_count is NULL), in the order the previous sort left
 *             them: d_order [nq][cap] uint32 (optional, NULL = identity), list entry j is element d_order[q][j] of the [nq][cap]
 *             arrays — pg_sort_scores_dev's order and d_order / d_out_fused / the rows of pg_recommend_candidates_dnn3_dev plug in
 *             as they are.  Per element: d_rows uint64 (global rows of t: the embeddings), d_score fp64 (Item.Score), d_source
 *             uint8 (optional; the fan-in's numbering).  d_enable [nq] uint8 (optional): the sort's Condition gate (:119-128), as
 *             pg_diversity_rules_dev takes it.  Padding — an entry at or beyond the count, an order value >= cap, a row UINT64_MAX
 *             or a row outside t — leaves the list first and appears in no output.
 *             The list is taken to be score-descending already (ItemRankScore ran before).  The stage does NOT re-sort where the
 *             reference calls sort.Sort (:123, :130, :302): Go's sort.Sort is unstable, so entries of equal score have no defined
 *             order in the reference; the order that arrives is kept.
 *   Scalars   gamma; topn (ctx.Size); window (<= 1 means 5, :356-359); normalize_emb, ensure_pos_similarity, use_ssd_star as
 *             pg_ssd; norm_quality_score 0 / 1 / 2; candidate_count, min_score_percent, abort_run_cnt (0 = off);
 *             filter_source_mask: bit s set = source s is among FilterRetrieveIds (a source >= 32, or no d_source, matches nothing).
 *   Answer    per request, DEFINED bit for bit, in this order:
 *               1. enable == 0, or abort_run_cnt > 0 and the number of real entries <= abort_run_cnt: the list as it is (:119-134).
 *               2. entries whose source is in filter_source_mask go to `backup`, in order; the rest is `selected` (:156-169).
 *               3. gamma == 0: `selected` as it is (:304-308).
 *               4. cuts (:312-331): if (candidate_count > 0 || min_score_percent > 0) and len > topn: with candidate_count > 0 the
 *                  list is cut to max(topn, candidate_count); with min_score_percent > 0 and still len > topn it is cut at the
 *                  first idx >= topn with score[idx] / score[0] < min_score_percent — the fp64 quotient as written, so a NaN
 *                  quotient does not cut.  What a cut removes is gone.
 *               5. normalisation of the cut list's scores (:366-391), bit for bit orc_ssd_quality: mode 1 = the sequential sum,
 *                  the mean, stat.PopMeanVariance's ss / comp chains with separate multiply and add, StdScore; mode 2 = min-max
 *                  from the first and the last entry with eps = 1e-6.  mean == 0 or variance == 0 (mode 1), span == 0 (mode 2):
 *                  the cut list is the result, unchanged.
 *               6. SSDWithSlidingWindow over the cut list, T = min(len, topn) picks.
 *               7. result = the picks (or the unchanged list of 1, 3 or 5), then `backup`.
 *   Out       d_out_pos [nq][cap] uint32: the result as indices into the [nq][cap] arrays (composed with d_order), UINT32_MAX
 *             behind the count; d_out_count [nq]; optional d_out_rows [nq][cap] uint64: the rows at those positions, UINT64_MAX
 *             behind the count; optional d_out_quality [nq][cap] fp64, by INPUT position: the ssd_quality_score of every entry of
 *             the cut list when mode 1 or 2 ran (not bailed), the quiet NaN everywhere else.  Every output element is written
 *             exactly once; no output may overlap an input.
 *   Limits    nq <= PG_SSD_STAGE_MAX_NQ, cap <= PG_SSD_STAGE_MAX_CAP; n_max = candidate_count > 0 ? min(cap, max(topn,
 *             candidate_count)) : cap, the host-side bound on a request's cut list, <= PG_SSD_STAGE_MAX_N; d1 = t's dim +
 *             ensure_pos_similarity in {64, 65, 128, 129} and the effective window <= 16 (the batched kernel's shapes).  Anything
 *             else, a filtered view and a table of >= 2^32 rows: PG_ERR_UNSUPPORTED by name, nothing enqueued.  topn == 0,
 *             norm_quality_score outside 0..2, nq or cap 0: PG_ERR_INVALID.
 *   Kernels   a list kernel (one workgroup per request: the split and the renumbering by wave ballots, the cuts, the
 *             normalisation — mode 1's chains on one lane, by specification sequential), ssd_prepare_kernel and
 *             ssd_kernel_grid<D1> with a count per request (every request its own workgroups, mailbox and barrier), an epilogue
 *             kernel (picks → positions, backup, padding, rows, quality).  pg_stats' ssd_grid_calls grows by one per call. */
#define PG_SSD_STAGE_MAX_NQ 256
#define PG_SSD_STAGE_MAX_CAP 16384
#define PG_SSD_STAGE_MAX_N 8192
int pg_ssd_sort_dev(pg_ctx* ctx, const pg_table* t, uint32_t nq, uint32_t cap, const uint32_t* d_order, const uint64_t* d_rows,
                    const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const uint8_t* d_enable, double gamma,
                    uint32_t topn, uint32_t window, int normalize_emb, int ensure_pos_similarity, int norm_quality_score,
                    int use_ssd_star, uint32_t candidate_count, double min_score_percent, uint32_t abort_run_cnt,
                    uint32_t filter_source_mask, uint32_t* d_out_pos, uint32_t* d_out_count, uint64_t* d_out_rows,
                    double* d_out_quality);

/* ---- shard group: one process, several GPUs --------------------------------------------------------
 * BASELINE.json configs[4] / SURVEY.md 8e behind the C ABI (a cgo host cannot join a torch.distributed job): the item
 * table in contiguous row ranges [g*N/G, (g+1)*N/G), one context per shard, model weights replicated.  devices[] may
 * name one device several times (logical shards on one GPU: tests).  Peer access is enabled between distinct
 * devices; the two exchanges of a step (per-shard top-k lists; owners' rank scores and DPP embeddings) are direct
 * peer stores ordered by HIP events — no collective library, no host synchronisation inside a step.  The tail of a
 * step (RankScore, sort, DPPSort, page) is spread over the shards by request: shard s finishes requests q = s (mod G). */
typedef struct pg_group pg_group;
int pg_group_create(const int* devices, uint32_t n_shards, pg_group** out);
int pg_group_destroy(pg_group* g);
uint32_t pg_group_size(const pg_group* g);
int pg_group_info(const pg_group* g, uint64_t* total_rows, uint32_t* dim);
pg_ctx* pg_group_ctx(pg_group* g, uint32_t shard);
pg_table* pg_group_table(pg_group* g, uint32_t shard);
int pg_group_table_create(pg_group* g, uint64_t total_rows, uint32_t dim);
int pg_group_table_fill_synthetic(pg_group* g, uint64_t seed, int normalize);
int pg_group_table_upload(pg_group* g, uint64_t row0, uint64_t nrows, const float* host_rows);   /* global rows */
int pg_group_model_load(pg_group* g, pg_model_kind kind, pg_prec prec, const void* blob, size_t len);
typedef struct {
    uint32_t k;                /* recall depth (RecallCount) */
    uint32_t dpp_candidates;   /* DPPSortConfig.CandidateCount; 0 = no DPP stage (the page is the head of the sorted list) */
    double   dpp_alpha;        /* DPPSortConfig.Alpha */
    uint32_t dpp_window;       /* DPPSortConfig.WindowSize (0 = 10) */
    int      dpp_normalize_emb;
} pg_group_plan;
/* nq requests through sharded recall → merge → owner-computes DNN3 rank → RankScore → ItemRankScore sort → DPPSort on
 * the first max(top_n, dpp_candidates) entries (sort/dpp_sort.go:271-351; ctx.Size = top_n).  Outputs [nq][top_n] in
 * page order: global row ids, recall / model / fused scores; out_count[q] (optional) = entries that are items.
 * Results are identical to the single-shard path (pg_recommend_dnn3_dev + pg_dpp on one table). */
int pg_group_recommend(pg_group* g, const pg_expr* e, const char* rank_var, const pg_group_plan* plan,
                       const float* user_vecs, uint32_t nq, uint32_t top_n, uint64_t* out_rows,
                       float* out_recall_scores, float* out_rank_scores, double* out_fused, uint32_t* out_count);
/* The same step in two halves, as pg_recommend_dnn3_begin / pg_recommend_end on one GPU: _begin enqueues the whole
 * step on every shard and returns at once (user_vecs are copied), _end waits for it, verifies every shard's recall
 * plan (re-running the step where one did not hold) and delivers the pages.  Up to two steps may be outstanding: each
 * shard runs them on two lanes (contexts with their own stream and scratch), so one batch's fusion / sort / DPP tail
 * overlaps the next batch's scans.  Every ticket must be ended; table / model changes need the group idle. */
typedef struct pg_group_ticket pg_group_ticket;
int pg_group_recommend_begin(pg_group* g, const pg_expr* e, const char* rank_var, const pg_group_plan* plan,
                             const float* user_vecs, uint32_t nq, uint32_t top_n, pg_group_ticket** out);
int pg_group_recommend_end(pg_group* g, pg_group_ticket* ticket, uint64_t* out_rows, float* out_recall_scores,
                           float* out_rank_scores, double* out_fused, uint32_t* out_count);
/* The first exchange of the sharded step (the reference's only fan-in is service/recall.go:126-150): every shard
 * sends the best ceil(k/G + 6 sqrt(k/G) + 8) entries of every request's list; a step in which some shard's last sent entry lies
 * inside a merged top-k is repeated with the whole lists.  out4 = {steps served, steps that had to be repeated, bytes one shard
 * sent to each peer in the last step, entries per request and shard in it}. */
int pg_group_exchange_stats(pg_group* g, uint64_t* out4);

/* The shard-side steps of the same flow as device-level calls, for a one-process-per-GPU host that runs the two
 * exchanges itself (pairec_amd/dist.py over torch.distributed / RCCL).  Everything is fixed-size and stays on the
 * stream: no counts travel to the host.
 *   pg_topk_merge_lists_dev   pg_topk_merge_dev with the input layout selectable: list_major = 1 takes
 *                             [nlists][nq][per_list], what an all-gather of per-shard [nq][per_list] blocks produces
 *   pg_owned_compact_dev      of the merged global rows [nq][k], the candidates whose rows live in `t`: their local row
 *                             indices and their slots q * k + j, compacted request by request (stable), and the CSR
 *                             offsets d_req_offsets[nq + 1] — inputs of pg_rank_dnn3_dev (pass n_items = nq * k, an upper bound)
 *   pg_scatter_f32_dev        d_out[d_slot[i]] = d_vals[i] for i < *d_total (= d_req_offsets[nq]); d_out is pre-zeroed by the
 *                             caller, the owners' slots are disjoint, so a sum all-reduce of the slabs is exact
 *   pg_dpp_candidates_dev     global rows and relevance (fused score) of the first n_cand entries of every sorted list
 *   pg_gather_owned_rows_dev  d_out[i][dim] = row d_global_rows[i] where this shard owns it; other rows are left as they are
 *   pg_dpp_batch_dev          DPPSort.KernelMatrix + DPPWithWindow for n_req independent requests of n candidates given as
 *                             embedding rows d_emb [n_req][n][dim]; d_out_idx [n_req][topn], d_out_count [n_req] */
int pg_topk_merge_lists_dev(pg_ctx* ctx, const uint64_t* d_rows, const float* d_scores, uint32_t nq, uint32_t nlists,
                            uint32_t per_list, int list_major, uint32_t k, uint64_t* d_out_rows, float* d_out_scores);
int pg_owned_compact_dev(pg_ctx* ctx, const pg_table* t, const uint64_t* d_rows, uint32_t nq, uint32_t k,
                         uint32_t* d_local, uint32_t* d_slot, uint32_t* d_req_offsets);
int pg_scatter_f32_dev(pg_ctx* ctx, const float* d_vals, const uint32_t* d_slot, const uint32_t* d_total, uint32_t cap,
                       float* d_out);
int pg_dpp_candidates_dev(pg_ctx* ctx, const uint32_t* d_order, const uint64_t* d_rows, const double* d_fused, uint32_t nq,
                          uint32_t k, uint32_t n_cand, uint64_t* d_c_rows, double* d_c_rel);
int pg_gather_owned_rows_dev(pg_ctx* ctx, const pg_table* t, const uint64_t* d_global_rows, uint32_t n, float* d_out);
int pg_dpp_batch_dev(pg_ctx* ctx, const float* d_emb, const double* d_rel, uint32_t n_req, uint32_t n, uint32_t dim,
                     double alpha, uint32_t topn, uint32_t window, int normalize_emb, uint32_t* d_out_idx,
                     uint32_t* d_out_count);
/* DPPSort.KernelMatrix alone (sort/dpp_sort.go:372-475, table path): d_out_L [n_req][n][n] = diag(r) F F^T diag(r) in fp64 for the
 * same inputs as pg_dpp_batch_dev — what its greedy part consumes, exposed so that the matrix can be checked bit for bit */
int pg_dpp_kernel_matrix_dev(pg_ctx* ctx, const float* d_emb, const double* d_rel, uint32_t n_req, uint32_t n, uint32_t dim,
                             double alpha, int normalize_emb, double* d_out_L);

/* ---- request coalescer --------------------------------------------------------------------------
 * The reference calls its plug-ins once per request from many goroutines at once: one IAlgorithm.Run per recall
 * (service/recall.go:129-145 → vector_recall.go:88), one per batch of BatchCount = 100 items and per algorithm
 * (service/rank/rank_service.go:264-289), across overlapping HTTP requests (SURVEY.md 8b "Threading").  A table
 * pass costs the same for 1 query as for 128, so the library batches across callers itself: the pg_coalescer_*
 * calls below are issued concurrently from any number of host threads, each with ONE request; they block while a
 * library-owned dispatcher thread forms a batch — up to max_batch requests; a partial batch goes out once the
 * device has nothing queued and its oldest request has waited max_wait_us — runs ONE table pass / ONE rank launch
 * for the whole batch on the context's stream, and hands every caller its slice.  Up to `depth` batches are in
 * flight, so the next batch is queued behind the running one.  Results are bit-identical to the same request
 * issued alone through pg_recall_topk / pg_rank_dnn3 / pg_recommend_dnn3_dev (scores do not depend on what else
 * shares a pass).  cgo note: the calling goroutine's OS thread is parked in a futex wait, not spinning.
 * A coalesced batch records none of its context's stage timers (pg_stats' last_recall_ms / last_rank_ms, pg_last_scan_kernel_ms
 * keep what the last direct call left; the byte count is kept up): each HIP event record is ~6 us of idle queue, 40-60 us of a
 * small batch's 1.3-1.8 ms.  PG_COALESCER_TIMERS=1 in the environment records them as direct calls do; pg_coalescer_stats'
 * device_ms (enqueue -> completion) is there either way. */
typedef struct pg_coalescer pg_coalescer;
typedef struct {
    uint32_t k;               /* recall depth (RecallConfig.RecallCount), fixed per coalescer: 1..16384            */
    uint32_t max_batch;       /* requests per table pass, 1..256 (<= 32 when dim > 128); 0 = the maximum           */
    uint32_t max_wait_us;     /* how long a request may wait for company while the device is idle; 0 = 100.  Only
                               * while company is likely: once the recent gap between arrivals exceeds it, a request
                               * that finds the device idle is dispatched at once                                    */
    uint32_t depth;           /* batches in flight, 1..4; 0 = 2                                                    */
    uint32_t max_top_n;       /* pg_coalescer_recommend: largest page a caller may ask for, <= k; 0 = k            */
    uint32_t max_rank_items;  /* pg_coalescer_rank*: most candidates in one call (BatchCount); 0 = k               */
    uint32_t timeout_us;      /* deadline of every call, from its arrival (eas/client.go:53-58, 100 ms there);
                                 0 = none.  A caller whose deadline passes returns PG_ERR_TIMEOUT; its batch still
                                 completes for the other callers, and later calls are served as usual             */
} pg_coalescer_config;
/* model / expr / rank_var may be NULL: then only pg_coalescer_recall (and pg_coalescer_rank_dnn3 with a model) work. */
int pg_coalescer_create(pg_ctx* ctx, const pg_table* t, const pg_model* m, const pg_expr* e, const char* rank_var,
                        const pg_coalescer_config* cfg, pg_coalescer** out);

/* A scene's whole plug-in set behind one coalescer — what recconf names per scene (RecallConfs, RankConf.RankAlgoList +
 * RankScore, SortNames; recconf/recconf.go:54-57,736-745), so that EVERY per-request plug-in call of the reference has a
 * coalesced single-request entry point below:
 *   algos[]            RankAlgoList: up to 4 rank algorithms, each scoring every candidate (rank_service.go:259-289) —
 *                      PG_MODEL_DNN3 over the table's rows, or PG_MODEL_FM_TWOTOWER whose item field ids are the integer
 *                      columns item_field_cols[n_item_fields] of `features` (keyed by the same rows); `name` is the
 *                      algorithm's name = its variable in RankScore (rank_service.go:312-335)
 *   rank_score         RankConf.RankScore over the algorithms' names and current_score (needed by pg_coalescer_recommend*)
 *   rerank             1: DPPSort behind the ItemRankScore sort (SortNames: [ItemRankScore, DPPSort]): the first
 *                      rerank_candidates = max(ctx.Size, CandidateCount) entries of every sorted list are the DPP
 *                      candidates (sort/dpp_sort.go:280-291), `dpp` carries alpha / window / normalize_emb /
 *                      norm_relevance_score, the page is DPPWithWindow's pick sequence; max_top_n <= rerank_candidates
 *   query_model        OnlineVectorRecall: a PG_MODEL_FM_TWOTOWER whose user tower turns a request's user features into
 *                      the query (pg_coalescer_online_recall); the table is then the item-embedding table (dim = t_out)
 *   trigger_table      I2IVectorRecall: where trigger rows are looked up (NULL = the table itself)
 *   max_rerank_items   pg_coalescer_dpp: most candidates in one call (0 = 1024); max_hook_dim: widest hook embedding (0 = none) */
typedef struct {
    const pg_model* model;
    const char* name;
    const pg_features* features;
    const int32_t* item_field_cols;
    const pg_item_rows* item_rows;   /* optional: the materialised records of (model, features, columns) — preferred when set */
    /* a multi-output model (PG_MODEL_DNN3_MULTI): the names of its pg_model_num_outputs() outputs; RankScore then reads
     * "<name>_<output>" per output (rank_service.go:315-319), pg_coalescer_recommend_ex returns one rank plane per output
     * (in list order, an algorithm's outputs adjacent), pg_coalescer_rank / _rank_dnn3 write out_scores[o * n + i].
     * NULL for single-output models; NULL for a multi-output one names its outputs "0", "1", … */
    const char* const* output_names;
} pg_rank_algo;
typedef struct {
    pg_coalescer_config base;
    const pg_rank_algo* algos;
    uint32_t n_algos;
    const pg_expr* rank_score;
    int rerank;
    uint32_t rerank_candidates;
    pg_dpp_options dpp;
    const pg_model* query_model;
    const pg_table* trigger_table;
    uint32_t max_rerank_items;
    uint32_t max_hook_dim;
} pg_scene_config;
int pg_coalescer_create_scene(pg_ctx* ctx, const pg_table* t, const pg_scene_config* cfg, pg_coalescer** out);
/* fails every waiting request with PG_ERR_INVALID, joins the worker threads, frees the buffers */
int pg_coalescer_destroy(pg_coalescer* c);
/* VectorRecall.GetCandidateItems → IAlgorithm.Run(VectorRequest{K, Vector}) for ONE user vector [dim]:
 * out_rows[k], out_scores[k] as pg_recall_topk, *out_count (optional) = valid entries. */
int pg_coalescer_recall(pg_coalescer* c, const float* query, uint64_t* out_rows, float* out_scores,
                        uint32_t* out_count);
/* I2IVectorRecall.GetCandidateItems for ONE trigger item (pg_i2i_recall with n = 1): the query is row `trigger_row` of
 * the scene's trigger table; rides the same table pass as the vector recalls of other callers. */
/* HologresVectorRecallV2 through the coalescer: one request per call, up to 128 share one screened pass (32 one pass of the
 * exact scan, where the table needs that: pg_recall_topk_l2); out_dist ascending. */
int pg_coalescer_recall_l2(pg_coalescer* c, const float* query, uint64_t* out_rows, float* out_dist, uint32_t* out_count);
/* pg_recall_topk_exclude for ONE request (BeVectorRecall with the User2ItemExposureFilter, be_vector_recall.go:63-95 /
 * berecall/user_item_exposure_filter.go:22-33): query [dim] and the n_excl global row ids this user has seen.  Enabled by the
 * context option "coalescer_max_exclude" (0..4096, default 0), read once when the coalescer is created; with it positive,
 * k + coalescer_max_exclude > 16384 fails the creation with PG_ERR_UNSUPPORTED, and every slot holds the over-fetched answer
 * ([max_batch][k + coalescer_max_exclude] rows and scores) and the lists — nothing is allocated without the option.
 * PG_ERR_UNSUPPORTED when the coalescer was created with 0, when n_excl exceeds the option, and for a group coalescer.  Such
 * requests wait in a queue of their own (as the squared-Euclidean recalls do); one batch is one recall job at the FIXED depth
 * k + coalescer_max_exclude — one depth, so the table's per-K threshold model does not alternate — the compaction, and the
 * usual [nq][k] copy-out; plain batches are untouched.  Counted under flavour 0.  The answer is bit for bit
 * pg_recall_topk_exclude's for the same request alone. */
int pg_coalescer_recall_exclude(pg_coalescer* c, const float* query, const uint64_t* excl_rows, uint32_t n_excl,
                                uint64_t* out_rows, float* out_scores, uint32_t* out_count);
int pg_coalescer_i2i_recall(pg_coalescer* c, uint32_t trigger_row, uint64_t* out_rows, float* out_scores,
                            uint32_t* out_count);
/* OnlineVectorRecall.GetCandidateItems for ONE user (pg_online_vector_recall with n_req = 1): user_vec[d_user] goes
 * through the scene's query_model user tower on the device, the embedding is the query. */
int pg_coalescer_online_recall(pg_coalescer* c, const float* user_vec, uint64_t* out_rows, float* out_scores,
                               uint32_t* out_count);
/* IAlgorithm.Run of rank algorithm `algo` (index into the scene's list) for ONE batch of n <= max_rank_items
 * candidates of one user (rank_service.go:273): cand_rows are local row indices, out_scores[n] in request order.
 * user_vec is [d_user] of that model; user_field_ids [n_user_fields] for an FM + two-tower model, else NULL.
 * Calls for one algorithm from any number of threads and requests become one launch. */
int pg_coalescer_rank(pg_coalescer* c, uint32_t algo, const float* user_vec, const int32_t* user_field_ids,
                      const uint32_t* cand_rows, uint32_t n, float* out_scores);
/* the same for the first DNN3 / the first FM + two-tower algorithm of the scene */
int pg_coalescer_rank_dnn3(pg_coalescer* c, const float* user_vec, const uint32_t* cand_rows, uint32_t n,
                           float* out_scores);
int pg_coalescer_rank_fm2t(pg_coalescer* c, const float* user_vec, const int32_t* user_field_ids,
                           const uint32_t* cand_rows, uint32_t n, float* out_scores);
/* The whole path for ONE request (what pg_recommend_dnn3_dev does for a batch): recall top-k → every rank algorithm →
 * RankScore → descending sort → (DPPSort when the scene has the stage); the caller receives the page of top_n <=
 * max_top_n entries — the head of the sorted list, or DPP's picks in pick order — as global row ids, recall scores,
 * model scores and fused scores, all [top_n], and *out_count (optional) = entries that are items.
 * pg_coalescer_recommend reports the first algorithm's scores; _ex takes the FM models' user field ids and reports
 * every algorithm's scores, out_rank_scores [n_algos][top_n]. */
int pg_coalescer_recommend(pg_coalescer* c, const float* user_vec, uint32_t top_n, uint64_t* out_rows,
                           float* out_recall_scores, float* out_rank_scores, double* out_fused,
                           uint32_t* out_count);
int pg_coalescer_recommend_ex(pg_coalescer* c, const float* user_vec, const int32_t* user_field_ids, uint32_t top_n,
                              uint64_t* out_rows, float* out_recall_scores, float* out_rank_scores, double* out_fused,
                              uint32_t* out_count);
/* DPPSort.Sort for ONE request (pg_dpp_ex; sort/sort.go:65-125 calls it once per request, requests overlap): calls
 * with the same candidate count and options share one batched launch (KernelMatrix for all of them, one wave per
 * request for the greedy part).  has_table = 1: embeddings are rows cand_rows[n] of the table; hook_emb as pg_dpp_ex. */
int pg_coalescer_dpp(pg_coalescer* c, const uint32_t* cand_rows, const double* rel, uint32_t n,
                     const pg_dpp_options* opt, const double* hook_emb, uint32_t* out_idx, uint32_t* out_count,
                     double* out_relevance);
/* ---- per-request calls over several GPUs ------------------------------------------------------------------------
 * (a) The sharded table (BASELINE.json configs[4]): a coalescer over a shard group — pg_coalescer_recommend takes ONE
 *     request, the library batches up to 256 of them into pg_group_recommend_begin / _end steps (two in flight, one per
 *     lane), DPPSort included when plan->dpp_candidates > 0.  Only pg_coalescer_recommend / _stats / _destroy apply.
 * (b) Replicas (the 51 GB table of configs[1] fits every GPU): a router over one coalescer per replica; each request
 *     goes to the replica with the fewest requests outstanding (ties: round robin), so per-request calls from one
 *     process reach all N GPUs with no data-path exchange at all.  The router does not own the coalescers. */
int pg_coalescer_create_group(pg_group* g, const pg_expr* e, const char* rank_var, const pg_group_plan* plan,
                              const pg_coalescer_config* cfg, pg_coalescer** out);
typedef struct pg_router pg_router;
int pg_router_create(pg_coalescer* const* replicas, uint32_t n, pg_router** out);
int pg_router_destroy(pg_router* r);
int pg_router_recommend(pg_router* r, const float* user_vec, uint32_t top_n, uint64_t* out_rows,
                        float* out_recall_scores, float* out_rank_scores, double* out_fused, uint32_t* out_count);
int pg_router_recall(pg_router* r, const float* query, uint64_t* out_rows, float* out_scores, uint32_t* out_count);
/* requests each replica has served so far, [n] */
int pg_router_stats(pg_router* r, uint64_t* out_served);

/* SSDSort.Sort for ONE request (pg_ssd): calls of equal shape share one launch — every request its own set of
 * single-wave workgroups with its own barrier.  Shapes: dim 64 / 128, window <= 16, n <= max_rerank_items (others:
 * PG_ERR_UNSUPPORTED, use pg_ssd).  Arguments and outputs as pg_ssd. */
int pg_coalescer_ssd(pg_coalescer* c, const uint32_t* cand_rows, const double* rel, uint32_t n, double gamma, uint32_t topn,
                     uint32_t window, int normalize_emb, int ensure_pos_similarity, int norm_quality_score, int use_ssd_star,
                     uint32_t* out_idx, uint32_t* out_count, double* out_quality);
typedef struct {
    uint64_t requests[6], batches[6];   /* per flavour: 0 recall (vector / i2i / online), 1 rank, 2 recommend, 3 dpp, 4 ssd, 5 reserved */
    uint64_t largest_batch[6];
    uint64_t replans;                   /* batches whose first recall plan did not hold and was re-run */
    uint64_t timeouts;                  /* calls that returned PG_ERR_TIMEOUT */
    double   device_ms[6];              /* summed enqueue → completion time of the batches */
} pg_coalescer_stats_t;
int pg_coalescer_stats(pg_coalescer* c, pg_coalescer_stats_t* out);

/* Deadline form of pg_recommend_end: waits at most timeout_us for the batch; PG_ERR_TIMEOUT leaves the ticket valid
 * (end it again later — every ticket must be ended). */
int pg_recommend_end_timed(pg_ctx* ctx, pg_ticket* ticket, uint32_t timeout_us, double* scan_ms);
/* Test aid: occupies the context's stream for `ms` milliseconds with a kernel that only watches the clock — what a
 * hung or slow device looks like to callers with a deadline. */
int pg_debug_stall(pg_ctx* ctx, uint32_t ms);

/* ---- stats ----------------------------------------------------------------------------------*/
typedef struct {
    uint64_t recall_calls, recall_rows_scanned, recall_rescans;
    uint64_t rank_calls, rank_items;
    uint64_t sort_calls, sort_items;
    double   last_recall_ms, last_rank_ms, last_sort_ms;   /* hipEvent-timed, device side */
    uint64_t recall_predicted;          /* batches whose screening threshold came from the table's threshold model and held */
    /* screened recalls whose first plan held: the (row, query) pairs the full pass handed to the exact fp32 re-scoring, and the
     * queries they belong to (suspects per answer = recall_suspects / recall_suspect_queries / K); the pairs a mid-batch pass's
     * 4-bit stage handed to its int8 stage; screened plans that overflowed (rows crowded within the screen's error of the K-th
     * score) and finished on the exact scan */
    uint64_t recall_suspects, recall_suspect_queries, recall_i4m_pairs, recall_screen_overflows;
    uint64_t recall_record_growths;     /* batches re-run with larger hit-record areas (the table keeps them) */
    uint64_t recall_rescored;           /* of recall_suspects, the pairs that reached the exact fp32 re-scoring (fewer where a table's
                                           crowded rows switched the two-digit refinement stage on, csrc/recall_r2.hip) */
    uint64_t sort_split_calls;          /* score sorts and top-K final orders that took the split sort (few lists of 1025 … 8192
                                           items: runs sorted wave by wave over the chip, csrc/split_sort.hpp) */
    /* SSD calls by the kernel that served them (csrc/ssd.hip; d1 = table dim + ensure_pos_similarity; one count per launch
     * sequence, so a coalesced batch of R requests counts once): the multi-workgroup kernel (d1 64 / 65 / 128 / 129 and
     * window <= 16), the one-workgroup register kernel (those widths, window > 16, n <= 2048), the one-workgroup generic kernel
     * (everything else up to 8192 x 320) */
    uint64_t ssd_grid_calls, ssd_reg_calls, ssd_generic_calls;
    /* DPP calls by the greedy kernel that served them (csrc/dpp.hip:dpp_run_locked; one count per launch sequence, so a batch of
     * R requests counts once; pg_dpp_kernel_matrix_dev runs no greedy kernel and counts nothing; window 0 means 10 before the
     * rule is applied): the one-wave kernel with eight items per lane (n <= 512 and window <= 16), the one-wave kernel with
     * sixteen (otherwise n <= 1024 and window <= 10), the one-workgroup kernel (everything else up to 8192 candidates) */
    uint64_t dpp_wave8_calls, dpp_wave16_calls, dpp_block_calls;
    /* rank calls by the kernel that served them (csrc/rank_mlp.hip: rank_dnn3_dev_locked, rank_fm2t_dev_locked; one count per
     * launch sequence; the seven sum to rank_calls): the weights-stationary DNN3 kernel (512-256, bf16), the register-stationary
     * ones (128-128, 256-128, 256-256, bf16), the LDS-stationary one (1024-512, bf16), the two-role kernel in split bf16, the
     * two-role kernel in an fp16 mode (its split-bf16 pass over the marked tiles belongs to the same sequence and is not counted
     * as x3), the per-wave two-tower kernel over item records, and the general mlp_kernel (every other DNN3 or two-tower call:
     * fp32, 64-wide tables, rank_no_ws, shapes without a kernel of their own) */
    uint64_t rank_ws_calls, rank_rs_calls, rank_ls_calls, rank_x3_calls, rank_h2_calls, rank_isw_calls, rank_mlp_calls;
} pg_stats_t;
int pg_stats(pg_ctx* ctx, pg_stats_t* out);
/* time (ms) of the dominant kernel of the last pg_recall_* call, measured with HIP events on the
 * context's stream around the scan launches only (bench.py's roofline figure) */
int pg_last_scan_kernel_ms(pg_ctx* ctx, double* out_ms, uint64_t* out_bytes);
/* Measured HBM read ceiling: streams the table's rows through a plain read-only kernel `reps` times
 * and returns the best rate in GB/s.  SURVEY.md 8(d) asks for the roofline fraction against a measured
 * streaming ceiling beside the nominal 8 TB/s. */
int pg_hbm_read_probe(pg_ctx* ctx, const pg_table* t, int reps, double* out_gbps);
/* The shadow the screened recall streams for this table, built now if it is not yet (it is otherwise built by
 * the first recall after an upload): *out_elem_bytes = 1 (int8: dim 128 with a value range one scale can serve),
 * 2 (bf16: dim 64, and heavy-tailed dim-128 tables), 0 when the table
 * is scanned exactly in fp32 (other dims, non-finite rows, no memory).  int8: *out_scale = the table's
 * quantisation step s (x ~ s X, X in [-127,127]), *out_resid = max over rows of ||x - s X||_2 as measured —
 * the two table-side terms of the screen's error bound; 0 otherwise.  Any out pointer may be NULL. */
int pg_table_screen_info(pg_ctx* ctx, const pg_table* t, int* out_elem_bytes, float* out_scale, float* out_resid);
/* Diagnostics of a table's derived state (what the screens' error bounds are made of).  Read-only with
 * respect to answers: both build and read exactly what a recall would build and stream.
 *   info     builds the parts of `parts` (PG_DERIVED_*) that are not built yet, through the functions the recall calls and in
 *            its order (the statistics and the main shadow first, always), and reports the scalars.  A part that cannot exist
 *            for this table says so in its flag and is no error: i4 / r2 / pred on dim != 128 or a non-finite table, r2 and
 *            pred on a bf16 main shadow, nx on a dim other than 64 / 128.  Flags and values of parts never asked for report
 *            the table's current state.  elem_bytes as pg_table_screen_info.
 *   read     copies elements [first, first + n) of one array (PG_DERIVED_ARR_*) to host memory.  Lengths, in elements:
 *            I8 [rows + 64][dim] int8; BF16 [rows + 64][dim] u16; BLKNORM2 [ceil(rows / 32)] f32 (with the bf16 shadow);
 *            I4 [rows + 64][16] u32; I4S [rows + 64] u32 (scale bf16 low half | residual bound bf16 high half);
 *            I8R [rows + 64][128] int8; NX [rows + 64] f32; NXMIN [ceil(rows / 32)] f32; PRED [128 + 128 * 128] f32 followed
 *            by 5 doubles, counted as 128 + 128 * 128 + 10 four-byte elements.  The 64 padding rows are readable (the
 *            streaming kernels read them).  PG_ERR_INVALID on a NULL argument, an unknown array, a range outside the array
 *            or an array that is not built (ask info first). */
enum {
    PG_DERIVED_STATS = 1, PG_DERIVED_I4 = 2, PG_DERIVED_R2 = 4, PG_DERIVED_NX = 8, PG_DERIVED_PRED = 16
};
enum {
    PG_DERIVED_ARR_I8 = 0, PG_DERIVED_ARR_BF16 = 1, PG_DERIVED_ARR_BLKNORM2 = 2, PG_DERIVED_ARR_I4 = 3, PG_DERIVED_ARR_I4S = 4,
    PG_DERIVED_ARR_I8R = 5, PG_DERIVED_ARR_NX = 6, PG_DERIVED_ARR_NXMIN = 7, PG_DERIVED_ARR_PRED = 8
};
typedef struct {
    int32_t elem_bytes, all_finite;            /* main shadow: 0 / 1 / 2; rows all finite with norm^2 < 3e38 */
    float max_norm, s8, resid8;                /* >= max ||x||; int8 scale; >= max ||x - s8 X8|| (int8 shadow only) */
    int32_t i4_ok;
    float rho4, rmax4, lam4;
    int32_t r2_ok;
    float s8r, resid2;
    int32_t nx_valid;
    float l2_slack;
    int32_t pred_model;
    uint64_t pred_n_sample, pred_stride;       /* the model's sample: rows min(s * stride, rows - 1), s < n_sample */
} pg_table_derived_t;
int pg_table_derived_info(pg_ctx* ctx, const pg_table* t, uint32_t parts, pg_table_derived_t* out);
int pg_table_derived_read(pg_ctx* ctx, const pg_table* t, int which, uint64_t first, uint64_t n, void* out);

#ifdef __cplusplus
}
#endif
#endif /* PAIREC_GPU_H */
