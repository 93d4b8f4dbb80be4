"""GPU tests of the fan-in merge and of the stages behind it (csrc/fanin.hip, pg_recommend_candidates_dnn3_dev)
against tests/fanin_ref.py = o.unique_filter: every output array is compared by bits, padding and counts included.  The sizes
sit on the kernel's edges — its chunk of 1 024 positions, the tier boundary of 8 192 candidates, the largest cap of 16 384 —
and the ids are chosen against the table's hash, which is restated here."""
import numpy as np
import pytest

import cf_ref
import fanin_ref as ref
import pairec_amd as pa
from oracle import oracle as o
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

U64MAX = ref.U64MAX
MAX_SOURCES, MAX_CAP, LDS_MAX_CAP, CHUNK = 8, 16384, 8192, 1024      # fanin.hip (test_fanin_cpu.py holds the header to them)
HASH_MUL = np.uint64(0x9E3779B97F4A7C15)                            # ... and its hash: (key * HASH_MUL mod 2^64) >> (64 - bits),
FUSION_TOL = 5e-15 * 5                                              # test_gpu_parity.py: the device pow's ulps against operands below 5


def table_bits(cap):
    """... over the power of two >= max(2 cap, 1024) slots; key = id - the request's smallest id (LDS tier) or the id (scratch)"""
    bits = 10
    while (1 << bits) < 2 * cap:
        bits += 1
    return bits


def slot(keys, bits):
    return (np.asarray(keys, np.uint64) * HASH_MUL) >> np.uint64(64 - bits)


def tier(ctx, lds):
    ctx.set_option("fanin_lds_max_cap", LDS_MAX_CAP if lds else 0)


def check(ctx, sources, optional=False):
    want = ref.merge(sources)
    got = ctx.fanin_merge(sources)
    ref.same(got, want)
    if optional:
        ref.same(ctx.fanin_merge(sources, recall_scores=False, source_mask=False), want, planes=False)
        part = ctx.fanin_merge(sources, recall_scores=True, source_mask=False)
        assert part[4] is None and np.array_equal(part[3].view(np.uint64), want[3].view(np.uint64))
    return got


def random_sources(rng, nq, ks, universe, row_offset=0, pad=0.05):
    src = []
    for i, k in enumerate(ks):
        rows = (rng.integers(0, universe, (nq, k)).astype(np.uint64) + np.uint64(row_offset))
        rows[rng.random((nq, k)) < pad] = U64MAX
        sc = rng.standard_normal((nq, k))
        src.append((rows, sc.astype(np.float32) if i % 2 == 0 else sc))
    return src


# ---- sizes, sources, the chunk and the tiers ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,ks", [(1, [1]), (1, [1000]), (3, [63, 64]), (3, [65, 1000, 64]), (256, [1, 63, 64, 65]),
                                   (3, [1, 63, 64, 65, 1000, 1, 63, 64]), (256, [64] * 8), (1, [1000] * 8)])
def test_sizes_and_sources(ctx, nq, ks):
    rng = np.random.default_rng(100 + nq + len(ks))
    check(ctx, random_sources(rng, nq, ks, max(2, sum(ks) // 2), row_offset=1 << 20), optional=True)


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("cap", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_chunk_boundary(ctx, cap, lds):
    rng = np.random.default_rng(cap)
    try:
        tier(ctx, lds)
        check(ctx, random_sources(rng, 3, [1000, cap - 1000], cap // 3, row_offset=7))
    finally:
        tier(ctx, True)


@pytest.mark.parametrize("cap", [LDS_MAX_CAP - 1, LDS_MAX_CAP, LDS_MAX_CAP + 1, MAX_CAP])
def test_tier_boundary_and_largest_cap(ctx, cap):
    rng = np.random.default_rng(cap)
    ks = [5000, 2000, cap - 7000] if cap < MAX_CAP else [2048] * 8
    # (few duplicates and many: the table of the larger universe runs at its full load)
    check(ctx, random_sources(rng, 2, ks, 4 * cap, row_offset=1 << 33))
    check(ctx, random_sources(rng, 1, ks, cap // 8, row_offset=3))


def test_argument_errors_leave_the_context_usable(ctx):
    d = ctx.malloc(1 << 16)
    ok = (d, d, 4, False)
    for sources, nq in (([], 1), ([ok] * 9, 1), ([ok, (d, d, 0, False)], 1), ([(d, d, MAX_CAP, True), (d, d, 1, True)], 1), ([ok], 0), ([ok], 257)):
        with pytest.raises(PgError) as ei:
            ctx.fanin_merge_dev(sources, nq, d, d, d, 0, 0, d)
        assert ei.value.code in (-1, -4) and "pg_fanin_merge_dev" in str(ei.value)
    with pytest.raises(PgError) as ei:
        ctx.fanin_merge_dev([ok], 1, 0, d, d, 0, 0, d)
    assert ei.value.code == -1
    ctx.free(d)
    check(ctx, random_sources(np.random.default_rng(1), 2, [5, 6], 8))


# ---- overlap -----------------------------------------------------------------------------------------------------------------------

def test_overlap_between_sources(ctx):
    rng = np.random.default_rng(2)
    nq, k = 3, 300
    a = np.stack([rng.permutation(5000)[:k] for _ in range(nq)]).astype(np.uint64)
    sc = lambda: rng.standard_normal((nq, k))                                        # noqa: E731
    disjoint = [(a, sc().astype(np.float32)), (a + np.uint64(5000), sc()), (a + np.uint64(10000), sc().astype(np.float32))]
    got = check(ctx, disjoint)
    assert got[5].tolist() == [3 * k] * nq and np.all(np.isin(got[4], (1, 2, 4)))
    identical = [(a, sc()), (a.copy(), sc().astype(np.float32))]
    got = check(ctx, identical)
    assert got[5].tolist() == [k] * nq and np.all(got[4][:, :k] == 3) and np.all(got[2][:, :k] == 0)
    perm = np.stack([rng.permutation(a[q]) for q in range(nq)])
    got = check(ctx, [(a, sc().astype(np.float32)), (perm, sc()), (perm[:, ::-1].copy(), sc())])
    assert np.array_equal(got[0][:, :k], a) and np.all(got[4][:, :k] == 7)
    pads = np.full((nq, 70), U64MAX, np.uint64)
    check(ctx, [(pads, rng.standard_normal((nq, 70))), (a, sc()), (pads.copy(), rng.standard_normal((nq, 70)).astype(np.float32)), (a, sc())])
    holes = a.copy()
    holes[:, 5:200:3] = U64MAX                                                       # padding in the middle of a list
    holes[1] = U64MAX                                                                # request 1: every entry of every source is padding
    got = check(ctx, [(holes, sc().astype(np.float32)), (holes[:, ::-1].copy(), sc())], optional=True)
    assert got[5][1] == 0 and np.all(got[0][1] == U64MAX) and np.all(got[2][1] == 0xFF) and np.all(got[4][1] == 0)


def test_duplicates_inside_one_source(ctx):
    rng = np.random.default_rng(3)
    ids = (rng.permutation(100000)[:1100] + 50).astype(np.uint64)
    twice = ids[:1000].copy().reshape(1, -1)
    twice[0, 10], twice[0, 500], twice[0, 501] = twice[0, 3], twice[0, 4], twice[0, 4]      # two times, three times
    twice[0, 999] = twice[0, 0]                                                             # first and last position of 1 000
    sc = np.arange(1000, dtype=np.float64).reshape(1, -1) + 0.5
    got = check(ctx, [(twice, sc)])
    assert got[5][0] == 996 and got[1][0, 0] == 0.5 and got[3][0, 0, 0] == 999.5            # Item.Score the first, RecallScores the last
    # ... the same lists behind and in front of another source, and an id on both sides of a chunk boundary (positions 1023 | 1024)
    other = ids[1000:1100].copy().reshape(1, -1)
    other[0, 23], other[0, 24], other[0, 50] = other[0, 0], other[0, 0], twice[0, 4]
    got = check(ctx, [(twice, sc.astype(np.float32)), (other, rng.standard_normal((1, 100)))])
    pos = int(np.nonzero(got[0][0] == other[0, 0])[0][0])
    assert got[4][0, pos] == 2 and got[2][0, pos] == 1
    check(ctx, [(other, rng.standard_normal((1, 100))), (twice, sc)])
    long = ids[:1030].copy().reshape(1, -1)
    long[0, 1024], long[0, 1029] = long[0, 1023], long[0, 1022]
    for lds in (True, False):
        try:
            tier(ctx, lds)
            check(ctx, [(long, rng.standard_normal((1, 1030)).astype(np.float32))])
            check(ctx, [(twice, sc), (other, rng.standard_normal((1, 100)).astype(np.float32)), (twice[:, ::-1].copy(), sc * 2)])
        finally:
            tier(ctx, True)


# ---- hostile ids -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", [True, False])
def test_ids_that_collide_in_the_table(ctx, lds):
    rng = np.random.default_rng(4)
    ks = [600, 400]
    bits = table_bits(sum(ks))
    base = np.uint64((1 << 40) + 12345) if lds else np.uint64(0)        # LDS keys are distances to the smallest id, scratch keys the ids
    keys = np.arange(1, 6_000_000, dtype=np.uint64)
    h = slot(keys, bits)
    one = keys[h == 77][:700]                                           # every id in ONE slot
    run = keys[(h >= 300) & (h < 340)][:700]                            # ... and in a run of adjacent slots
    assert one.size == 700 and run.size == 700
    srcs = []
    for pool in (one, run):
        a = np.concatenate([[0], rng.choice(pool, ks[0] - 1, replace=False)]).astype(np.uint64) + base      # (key 0: the smallest id itself)
        b = rng.choice(pool, ks[1], replace=True).astype(np.uint64) + base
        srcs.append([(a.reshape(1, -1), rng.standard_normal((1, ks[0]))), (b.reshape(1, -1), rng.standard_normal((1, ks[1])).astype(np.float32))])
    both = [(np.concatenate([srcs[0][i][0], srcs[1][i][0]]), np.concatenate([srcs[0][i][1], srcs[1][i][1]])) for i in range(2)]
    try:
        tier(ctx, lds)
        got = check(ctx, both)
        assert got[5][0] < 1000 and got[5][1] < 1000                    # (duplicates took part)
    finally:
        tier(ctx, True)


def test_ids_equal_modulo_2_32_and_id_0(ctx):
    rng = np.random.default_rng(5)
    off = np.uint64((1 << 33) + (1 << 20))
    low = rng.permutation(1 << 16)[:200].astype(np.uint64)
    a = (low + off).reshape(1, -1)
    b = (low + off + np.uint64(1 << 32)).reshape(1, -1)                 # differ from a's only above bit 32
    c = (low[::-1] + off + np.uint64(1 << 34)).reshape(1, -1)
    sc = lambda: rng.standard_normal((1, 200))                          # noqa: E731
    got = check(ctx, [(a, sc()), (b, sc().astype(np.float32)), (c, sc()), (a.copy(), sc())])
    assert got[5][0] == 600
    # ids that fit 32-bit distances, far above 2^33: the LDS tier's keys
    got = check(ctx, [(a, sc()), (a + np.uint64(100), sc()), (a[:, ::-1].copy(), sc().astype(np.float32))])
    assert got[5][0] == np.unique(np.concatenate([a[0], a[0] + np.uint64(100)])).size
    # id 0, beside the largest ids there are
    z = np.array([[0, 5, 0, U64MAX - 1, U64MAX, 5, U64MAX - 1, 0]], np.uint64)
    got = check(ctx, [(z, np.arange(8, dtype=np.float64).reshape(1, -1)), (z[:, ::-1].copy(), np.arange(8, dtype=np.float32).reshape(1, -1))])
    assert got[0][0, :3].tolist() == [0, 5, U64MAX - 1] and got[5][0] == 3
    z2 = np.array([[0, 3, 0, 1, 3]], np.uint64)
    check(ctx, [(z2, np.arange(5, dtype=np.float64).reshape(1, -1))])


def test_score_bits_travel_untouched(ctx):
    f64 = np.array([0x7FF8000000000001, 0x7FF4DEADBEEF0001, 0xFFF8000000000123, 0x7FF0000000000000, 0xFFF0000000000000,
                    0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x3FF0000000000001,
                    0x7FEFFFFFFFFFFFFF, 0x0000000000000000], np.uint64).view(np.float64)
    f32 = np.array([0x7FC00001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,
                    0x00800000, 0x7F7FFFFF, 0x3F800001], np.uint32).view(np.float32)
    n = f64.size
    ids = np.arange(10, 10 + n, dtype=np.uint64)
    # every special value as a first occurrence, as a duplicate's recall score, and as the last of two inside one source
    srcs = [(ids.reshape(1, -1), f32.reshape(1, -1)), (ids[::-1].reshape(1, -1).copy(), f64.reshape(1, -1)),
            (np.concatenate([ids, ids]).reshape(1, -1), np.concatenate([f32[::-1], np.roll(f32, 3)]).reshape(1, -1)),
            (np.concatenate([ids + np.uint64(100), ids]).reshape(1, -1), np.concatenate([f64, np.roll(f64, 5)]).reshape(1, -1))]
    got = check(ctx, srcs, optional=True)
    assert np.array_equal(got[1][0, :n].view(np.uint64), f32.astype(np.float64).view(np.uint64))
    assert np.array_equal(got[3][1, 0, :n].view(np.uint64), f64[::-1].view(np.uint64))
    check(ctx, srcs[::-1])


# ---- three recalls of one table, merged and ranked ---------------------------------------------------------------------------------

N, DIM, NQ = 20000, 128, 5
K_VEC, K_I2I, K_CF = 300, 100, 200
RANK_SCORE = "${gpu_dnn}*(1+${current_score})^0.1"


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    rng = np.random.default_rng(6)
    s = Scene()
    s.t = pa.Table(ctx, N, DIM)
    s.t.fill_synthetic(o.SEED_TABLE)
    s.tab = o.synth_rows(o.SEED_TABLE, 0, N, DIM)
    s.users = o.synth_rows(o.SEED_QUERY, 3, NQ, DIM)
    s.w = o.Dnn3Weights()
    s.m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(s.w.w1, s.w.b1, s.w.w2, s.w.b2, s.w.w3, s.w.b3, 128))
    # a small similarity table: rows 0 .. 399 have lists of 60 neighbours among the rows the vector recall tends to return too
    vec_rows, _ = o.recall_topk(s.tab, s.users, K_VEC)
    pool = np.unique(np.concatenate([vec_rows.reshape(-1).astype(np.int64), rng.integers(0, N, 600)]))
    s.sim = pa.SimTable(ctx, s.t)
    s.sim_host = cf_ref.SimLists(N, 0)
    off = np.arange(401, dtype=np.uint64) * np.uint64(60)
    nb = np.concatenate([rng.choice(pool, 60, replace=False) for _ in range(400)]).astype(np.uint32)
    sm = rng.uniform(0.05, 1.0, nb.size).astype(np.float32)
    s.sim.upload(off, nb, sm, 0)
    s.sim_host.upload(off, nb, sm, 0)
    s.trig = [rng.choice(400, 12, replace=False).astype(np.uint32) for _ in range(NQ)]
    s.pref = [rng.uniform(0.1, 3.0, 12) for _ in range(NQ)]
    s.i2i_trig = vec_rows[:, 0].astype(np.uint32)                       # each user's best item is the I2I trigger
    # the oracle's three answers and their merge
    i2i_rows, i2i_sc = o.recall_topk(s.tab, s.tab[s.i2i_trig.astype(np.int64)], K_I2I)
    cf_rows, cf_sc, cf_cnt = cf_ref.cf_recall(s.sim_host, s.trig, s.pref, K_CF, True)
    _, vec_sc = o.recall_topk(s.tab, s.users, K_VEC)
    s.oracle_sources = [(vec_rows.astype(np.uint64), vec_sc), (cf_rows, cf_sc), (i2i_rows.astype(np.uint64), i2i_sc)]
    s.want = ref.merge(s.oracle_sources)
    # the device's: every list stays in device memory between its recall and the merge
    cap = K_VEC + K_CF + K_I2I
    s.cap = cap
    d_users = ctx.to_device(s.users)
    d_vr, d_vs = ctx.malloc(NQ * K_VEC * 8), ctx.malloc(NQ * K_VEC * 4)
    s.t.recall_topk_dev(d_users, NQ, K_VEC, d_vr, d_vs)
    toff = (np.arange(NQ + 1) * 12).astype(np.uint32)
    d_tr, d_pf = ctx.to_device(np.concatenate(s.trig)), ctx.to_device(np.concatenate(s.pref))
    d_cr, d_cs = ctx.malloc(NQ * K_CF * 8), ctx.malloc(NQ * K_CF * 8)
    s.sim.cf_recall_dev(d_tr, d_pf, toff, K_CF, d_cr, d_cs, True)
    ir, isc, _ = s.t.i2i_recall(s.i2i_trig, K_I2I)
    d_ir, d_is = ctx.to_device(ir), ctx.to_device(isc)
    outs = [np.empty((NQ, cap), np.uint64), np.empty((NQ, cap), np.float64), np.empty((NQ, cap), np.uint8),
            np.empty((3, NQ, cap), np.float64), np.empty((NQ, cap), np.uint32), np.empty(NQ, np.uint32)]
    d_out = [ctx.malloc(a.nbytes) for a in outs]
    ctx.fanin_merge_dev([(d_vr, d_vs, K_VEC, False), (d_cr, d_cs, K_CF, True), (d_ir, d_is, K_I2I, False)], NQ, *d_out)
    ctx.synchronize()
    for a, p in zip(outs, d_out):
        ctx.d2h(a, p)
    s.got = tuple(outs)
    for p in [d_users, d_vr, d_vs, d_tr, d_pf, d_cr, d_cs, d_ir, d_is] + d_out:
        ctx.free(p)
    yield s
    s.sim.destroy()
    s.m.destroy()
    s.t.destroy()


def test_three_recalls_merged_on_the_device(scene):
    ref.same(scene.got, scene.want)
    cnt = scene.got[5]
    assert np.all(cnt < scene.cap) and np.all(cnt > K_VEC)             # the recalls overlap, and none is contained in another
    shared = (scene.got[4] & (scene.got[4] - 1)) != 0                   # items more than one recall found, in every request
    assert np.all(shared.any(axis=1))


def test_candidates_rank_fuse_sort_against_the_oracle(ctx, scene):
    rows, score, _, _, _, cnt = scene.want
    ex = pa.Expr(RANK_SCORE)
    rk, fu, order = pa.recommend_candidates_dnn3(ctx, scene.t, scene.m, ex, "gpu_dnn", scene.users, rows, score, cnt)
    ex.free()
    for q in range(NQ):
        c = int(cnt[q])
        local = rows[q, :c].astype(np.uint32)
        # PREC_F32: the model scores of pg_rank_dnn3 on the same rows, bit for bit; padding slots 0 / NaN
        rk2 = scene.m.rank_dnn3(scene.t, scene.users[q:q + 1], local, np.array([0, c], np.uint32))
        assert np.array_equal(rk[q, :c].view(np.uint32), rk2.view(np.uint32))
        assert np.all(rk[q, c:].view(np.uint32) == 0) and np.all(fu[q, c:].view(np.uint64) == ref.NAN_BITS)
        items = []
        for j in range(c):
            it = o.OracleItem(str(rows[q, j]), score[q, j], "s")
            it.add_algo_score("gpu_dnn", float(rk[q, j]))
            items.append(it)
        o.fuse_scores(RANK_SCORE, items)
        want = np.array([it.score for it in items])
        assert np.max(np.abs(fu[q, :c] - want)) <= FUSION_TOL
        # ItemRankScore over the real candidates, the padding slots behind them
        assert np.array_equal(order[q, :c], o.sort_scores(fu[q, :c], True))
        assert sorted(order[q, c:].tolist()) == list(range(c, scene.cap))


def test_current_score_keeps_all_64_bits(ctx, scene):
    rows, score, source, _, _, cnt = scene.want
    cf = (source == 1) & (score.astype(np.float32).astype(np.float64) != score)
    assert np.count_nonzero(cf) > 100                                   # collaborative-filter scores no float32 holds
    ex = pa.Expr("${current_score}")
    _, fu, order = pa.recommend_candidates_dnn3(ctx, scene.t, scene.m, ex, "gpu_dnn", scene.users, rows, score, cnt)
    ex.free()
    for q in range(NQ):
        c = int(cnt[q])
        assert np.array_equal(fu[q, :c].view(np.uint64), score[q, :c].view(np.uint64))
        assert np.array_equal(order[q, :c], o.sort_scores(score[q, :c], True))
    # without counts the rows alone mark the padding; a row outside the table is padding too
    r2 = rows.copy()
    r2[0, 1] = N + 5
    ex = pa.Expr("${current_score}")
    _, fu2, _ = pa.recommend_candidates_dnn3(ctx, scene.t, scene.m, ex, "gpu_dnn", scene.users, r2, score)
    ex.free()
    assert fu2.view(np.uint64)[0, 1] == ref.NAN_BITS and fu2.view(np.uint64)[0, 0] == score.view(np.uint64)[0, 0]
    assert np.all(fu2[:, -1].view(np.uint64) == ref.NAN_BITS)


def test_one_vector_recall_reproduces_recommend_dnn3(ctx, scene):
    ex = pa.Expr(RANK_SCORE)
    rows, sc, rk, fu, order, cnt = pa.recommend_dnn3(ctx, scene.t, scene.m, ex, "gpu_dnn", scene.users, K_VEC)
    rk2, fu2, order2 = pa.recommend_candidates_dnn3(ctx, scene.t, scene.m, ex, "gpu_dnn", scene.users, rows, sc.astype(np.float64), cnt)
    ex.free()
    assert np.array_equal(rk.view(np.uint32), rk2.view(np.uint32))
    assert np.array_equal(fu.view(np.uint64), fu2.view(np.uint64))
    assert np.array_equal(order, order2)


def test_candidates_refuse_a_view_and_a_division_by_zero(ctx, scene):
    rows, score, _, _, _, cnt = scene.want
    feats = pa.Features(ctx, N)
    feats.set_column("cat", pa.F_I32, (np.arange(N) % 4).astype(np.int32))
    v = scene.t.view(feats, "cat", "==", 1)
    ex = pa.Expr(RANK_SCORE)
    with pytest.raises(PgError) as ei:
        pa.recommend_candidates_dnn3(ctx, v, scene.m, ex, "gpu_dnn", scene.users, rows, score, cnt)
    assert ei.value.code == -4 and "view" in str(ei.value)
    z = pa.Expr("${gpu_dnn}/(${current_score}-${current_score})")
    with pytest.raises(PgError) as ei:
        pa.recommend_candidates_dnn3(ctx, scene.t, scene.m, z, "gpu_dnn", scene.users, rows, score, cnt)
    assert ei.value.code == -5
    pa.recommend_candidates_dnn3(ctx, scene.t, scene.m, ex, "gpu_dnn", scene.users, rows, score, cnt)      # the context serves on
    for e in (ex, z):
        e.free()
    v.destroy()
    feats.destroy()
