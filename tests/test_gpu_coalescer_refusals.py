"""What the request coalescer refuses, and in which words: the return code and the exact pg_last_error text of every refusal of
pg_coalescer_create[_scene] and of the per-request entry points that is not pinned elsewhere.  A 512-row x 64-dim table, k = 8,
max_batch = 4, the smallest DNN3 the loader takes ([64+64]->128->128->1).  Every creation here is refused before anything is
allocated; every call is refused before it is queued (the coalescers' statistics stay at zero), so creating the two coalescers
(ensure_table_stats) is the only device work."""
import ctypes as C

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

N, D, K, MAX_BATCH = 512, 64, 8, 4
INVALID, UNSUPPORTED = -1, -4
EXPR = "${gpu_dnn}*(1+${current_score})^0.1"


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def world(ctx):
    t = pa.Table(ctx, N, D)
    t.fill_synthetic(o.SEED_TABLE)
    w = o.Dnn3Weights(d_user=D, d_item=D, h1=128, h2=128)
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, D))
    multi = {}
    for n_out in (2, 4, 8):
        wm = o.Dnn3MultiWeights(n_out, d_user=D, d_item=D, h1=128, h2=128)
        multi[n_out] = pa.RankModel(ctx, pa.MODEL_DNN3_MULTI, pa.PREC_F32, pa.pack_dnn3_multi(wm.w1, wm.b1, wm.w2, wm.b2, wm.w3m, wm.b3m, D))
    ex = pa.Expr(EXPR)
    yield {"t": t, "m": m, "multi": multi, "ex": ex}
    ex.free()
    for mm in [m] + list(multi.values()):
        mm.destroy()
    t.destroy()


def _refused(code, text, call):
    with pytest.raises(pa._lib.PgError) as e:
        call()
    print(e.value.code, str(e.value))
    assert e.value.code == code and str(e.value) == "pairec_gpu error %d: %s" % (code, text)


def test_creation_refusals(ctx, world):
    t, m, multi, ex = world["t"], world["m"], world["multi"], world["ex"]

    def create(k=K, **kw):
        kw.setdefault("max_batch", MAX_BATCH)
        return lambda: pa.Coalescer(ctx, t, k, **kw)

    _refused(INVALID, "pg_coalescer_create: depth 5 (at most 4)", create(depth=5))
    _refused(INVALID, "pg_coalescer_create: max_top_n 9 exceeds k 8", create(max_top_n=9))
    _refused(INVALID, "pg_coalescer_create: max_batch 257 exceeds 256 queries per pass at dim 64", create(max_batch=257))
    _refused(INVALID, "pg_coalescer_create: a RankScore expression needs at least one rank algorithm", create(algos=[], expr=ex))
    _refused(INVALID, "pg_coalescer_create: a RankScore expression needs a model and its name", create(expr=ex))
    _refused(INVALID, "pg_coalescer_create: the scene's models have more than 12 outputs together",
             create(algos=[("a", multi[8]), ("b", multi[4]), ("c", m)]))
    _refused(INVALID, "pg_coalescer_create: \"a\": output 1 has no name", create(algos=[("a", multi[2], ["ctr", ""])]))
    _refused(INVALID, "pg_coalescer_create: the DPP stage sits behind a RankScore sort", create(dpp={"candidates": 4}))
    _refused(INVALID, "pg_coalescer_create: max_top_n 6 exceeds rerank_candidates 4 (DPP candidates = max(ctx.Size, CandidateCount) "
             "must not depend on the request)", create(algos=[("gpu_dnn", m)], expr=ex, dpp={"candidates": 4}, max_top_n=6))
    ctx.set_option("coalescer_max_exclude", 4096)
    try:
        _refused(UNSUPPORTED, "pg_coalescer_create: k=12289 plus coalescer_max_exclude=4096 exceeds the recalls' depth of 16384", create(k=12289))
        # which check wins when several fail: the order of the checks
        _refused(INVALID, "pg_coalescer_create: depth 5 (at most 4)", create(k=12289, depth=5, max_top_n=12290))
        _refused(INVALID, "pg_coalescer_create: \"a\": output 1 has no name", create(k=12289, algos=[("a", multi[2], ["ctr", ""])]))
    finally:
        ctx.set_option("coalescer_max_exclude", 0)


def test_entry_point_refusals(ctx, world):
    t, m, ex = world["t"], world["m"], world["ex"]
    L = ctx.L
    ctx.set_option("coalescer_max_exclude", 2)                   # (read once, at creation)
    try:
        scene = pa.Coalescer(ctx, t, K, algos=[("gpu_dnn", m)], expr=ex, max_batch=MAX_BATCH, depth=1, max_top_n=4, max_rank_items=8,
                             max_rerank_items=16)
    finally:
        ctx.set_option("coalescer_max_exclude", 0)
    plain = pa.Coalescer(ctx, t, K, max_batch=MAX_BATCH, depth=1)
    u = np.zeros(D, np.float32)
    rows, rec, rnk, fus, cnt = np.zeros(K, np.uint64), np.zeros(K, np.float32), np.zeros(K, np.float32), np.zeros(K, np.float64), C.c_uint32()

    def recommend(co, top_n):
        return lambda: pa._lib.check(L.pg_coalescer_recommend(co.h, _ptr(u), top_n, _ptr(rows), _ptr(rec), _ptr(rnk), _ptr(fus), C.byref(cnt)))

    try:
        _refused(INVALID, "pg_coalescer_recommend: top_n 0 outside 1..4", recommend(scene, 0))
        _refused(INVALID, "pg_coalescer_recommend: top_n 5 outside 1..4", recommend(scene, 5))
        _refused(INVALID, "pg_coalescer_recommend: the coalescer was created without a RankScore expression", recommend(plain, 1))
        _refused(INVALID, "pg_coalescer_rank: 9 candidates exceed max_rank_items 8", lambda: scene.rank_dnn3(u, np.arange(9)))
        _refused(INVALID, "pg_coalescer_rank: candidate 1 row 512 outside table of 512 rows", lambda: scene.rank_dnn3(u, [0, N]))
        _refused(INVALID, "pg_coalescer_online_recall: the scene has no query model", lambda: scene.online_recall(u))
        _refused(UNSUPPORTED, "pg_coalescer_recall_exclude: a list of 3 ids; the coalescer was created with coalescer_max_exclude = 2",
                 lambda: scene.recall_exclude(u, [1, 2, 3]))
        _refused(UNSUPPORTED, "pg_coalescer_recall_exclude: a list of 1 ids; the coalescer was created with coalescer_max_exclude = 0",
                 lambda: plain.recall_exclude(u, [1]))
        _refused(UNSUPPORTED, "pg_coalescer_dpp: 17 candidates / hook width 0 exceed the scene's max_rerank_items 16 / max_hook_dim 0",
                 lambda: scene.dpp(np.arange(17), np.ones(17), 1.0, 4, 4))
        for co in (scene, plain):                                # no refused call was queued
            s = co.stats()
            assert list(s.requests) == [0] * 6 and list(s.batches) == [0] * 6 and s.timeouts == 0
    finally:
        scene.destroy()
        plain.destroy()
