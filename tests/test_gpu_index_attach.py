"""GPU tests of serving through an attached index (pg_index_attach): every recall job of the table — plain calls,
the coalescer's batches, the recommend pipeline — tries the index's enqueue-only plan first, and every answer equals, bit for bit,
the same call on the same table before attaching and the CPU oracle.  Stale indexes, dense batches, the round budget, non-finite
queries, detaching and the refusals are covered; so are two contexts on one attached index."""
import ctypes as C
import threading

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

N, D, CENTRES, SIGMA = 2_000_000, 128, 200, 0.1
N64 = 500_000
SEED = 0x1D0002
DENSE_DEFAULT = 0.01
KS = (1, 100, 5000)
NQS = (1, 7, 32, 64, 200, 256)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """two (rows, scores, counts) results are identical: ids, order, score bits, counts"""
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(np.asarray(a[2]), np.asarray(b[2]))


def like_oracle(got, orow, osc):
    assert np.array_equal(got[0], orow)
    assert np.array_equal(bits(got[1]), bits(osc))


def serving(ix, before=None):
    s = ix.serving_stats()
    return s if before is None else {k: s[k] - before[k] for k in s}


class options:
    """pg_set_option values for the duration of a block (restored to the given defaults)"""

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, (v, _) in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *a):
        for k, (_, d) in self.kv.items():
            self.ctx.set_option(k, d)


def wide(ctx):
    # the dense rule is calibrated at 100 M rows: lifted so that the plan serves on these small tables
    return options(ctx, index_dense_fraction=(1e6, DENSE_DEFAULT))


def run_threads(n, fn):
    errs = []
    gate = threading.Barrier(n)

    def wrap(i):
        try:
            gate.wait()
            fn(i)
        except BaseException as e:      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=wrap, args=(i,)) for i in range(n)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise errs[0]


def dev_recall(ctx, t, q, k, l2=False, c=None):
    c = c or ctx
    nq = q.shape[0]
    dq = ctx.to_device(np.ascontiguousarray(q, np.float32))
    dr, ds = ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 4)
    cnt = np.zeros(nq, np.uint32)
    fn = c.L.pg_recall_topk_l2_dev if l2 else c.L.pg_recall_topk_dev
    try:
        pa._lib.check(fn(c.h, t.h, C.c_void_p(dq), nq, k, C.c_void_p(dr), C.c_void_p(ds), cnt.ctypes.data))
        rows, sc = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32)
        ctx.d2h(rows, dr)
        ctx.d2h(sc, ds)
    finally:
        for p in (dq, dr, ds):
            ctx.free(p)
    return rows, sc, cnt


def host_recall(c, t, q, k):
    """pg_recall_topk on context c"""
    q = np.ascontiguousarray(q, np.float32)
    nq = q.shape[0]
    rows, sc, cnt = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32), np.zeros(nq, np.uint32)
    pa._lib.check(c.L.pg_recall_topk(c.h, t.h, q.ctypes.data, nq, k, rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
    return rows, sc, cnt


@pytest.fixture(scope="module")
def world(ctx):
    t = pa.Table(ctx, N, D)
    t.fill_mixture(SEED, CENTRES, SIGMA)
    tab = o.synth_mixture_rows(SEED, 0, N, D, CENTRES, SIGMA)
    q = o.synth_mixture_rows(SEED, 777, 256, D, CENTRES, SIGMA, stream=1)
    ip = o.recall_topk(tab, q, 5000)
    l2 = o.recall_topk_l2(tab, q, 5000)
    ix = pa.Index(ctx, t)
    yield t, tab, q, ip, l2, ix
    if ix.h:
        try:
            ix.detach()
        except pa._lib.PgError:
            pass
        ix.destroy()
    t.destroy()


def test_direct_calls_through_the_attached_index(ctx, world):
    t, tab, q, (orow, osc), (lrow, lsc), ix = world
    t64 = pa.Table(ctx, N64, 64)
    t64.fill_mixture(SEED + 1, CENTRES, SIGMA)
    tab64 = o.synth_mixture_rows(SEED + 1, 0, N64, 64, CENTRES, SIGMA)
    q64 = o.synth_mixture_rows(SEED + 1, 5, 256, 64, CENTRES, SIGMA, stream=1)
    o64, l64 = o.recall_topk(tab64, q64, 5000), o.recall_topk_l2(tab64, q64, 5000)
    ix64 = pa.Index(ctx, t64)
    cases = []
    for tt, qq, (ir, isc), (lr, ls) in ((t, q, (orow, osc), (lrow, lsc)), (t64, q64, o64, l64)):
        for nq in NQS:
            for k in KS:
                cases.append((tt, qq[:nq], k, False, ir[:nq, :k], isc[:nq, :k]))
                cases.append((tt, qq[:nq], k, True, lr[:nq, :k], ls[:nq, :k]))

    def call(tt, qq, k, l2, dev):
        if dev:
            return dev_recall(ctx, tt, qq, k, l2)
        return tt.recall_topk_l2(qq, k) if l2 else tt.recall_topk(qq, k)

    with wide(ctx):
        before = [call(tt, qq, k, l2, dev) for (tt, qq, k, l2, _, _) in cases for dev in (False, True)]
        ix.attach()
        ix64.attach()
        s0, s64, p0 = serving(ix), serving(ix64), ix.stats()
        after = [call(tt, qq, k, l2, dev) for (tt, qq, k, l2, _, _) in cases for dev in (False, True)]
        d, d64, p1 = serving(ix, s0), serving(ix64, s64), ix.stats()
        ix64.detach()
    i = 0
    for (tt, qq, k, l2, er, es) in cases:
        for dev in (False, True):
            same(after[i], before[i])
            like_oracle(after[i], er, es)
            i += 1
    # squared Euclidean batches of more than 128 queries run as two jobs
    jobs = sum((2 if (l2 and qq.shape[0] > 128) else 1) * 2 for (tt, qq, k, l2, _, _) in cases if tt is t)
    assert d["plans"] == jobs and d["plans_held"] == d["plans"], d
    assert d64["plans"] > 0 and d64["plans_held"] == d64["plans"], d64
    assert d["skipped_stale"] == 0 and d["skipped_switch"] == 0
    pairs = p1["pairs_scored"] - p0["pairs_scored"]
    assert 0 < pairs <= 0.06 * N * (p1["queries"] - p0["queries"]), pairs
    assert p1["calls"] - p0["calls"] == jobs
    ix64.destroy()
    t64.destroy()


def test_coalescer_through_the_attached_index(ctx, world):
    t, tab, q, (orow, osc), (lrow, lsc), ix = world
    k, top_n, callers = 100, 50, 48
    w = o.Dnn3Weights()
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128))
    ex = pa.Expr("${gpu_dnn}*(1+${current_score})^0.1")
    qs = q[:callers]
    trig = np.arange(callers, dtype=np.uint32) * 40_009 % N
    ref_ip = t.recall_topk(qs, k)
    ref_l2 = t.recall_topk_l2(qs, k)
    ref_i2i = t.i2i_recall(trig, k)
    ref_rec = []
    for i in range(callers):
        rows, rec, rnk, fus, order, cnt = pa.recommend_dnn3(ctx, t, m, ex, "gpu_dnn", qs[i:i + 1], k)
        p = order[0][:top_n]
        ref_rec.append((rows[0][p], rec[0][p], rnk[0][p], fus[0][p]))
    with wide(ctx):
        ix.attach()
        s0 = serving(ix)
        co = pa.Coalescer(ctx, t, k, m, ex, "gpu_dnn", max_top_n=top_n, max_wait_us=2000)
        try:
            got = {}
            run_threads(callers, lambda i: got.__setitem__(("ip", i), co.recall(qs[i])))
            run_threads(callers, lambda i: got.__setitem__(("l2", i), co.recall_l2(qs[i])))
            run_threads(callers, lambda i: got.__setitem__(("i2i", i), co.i2i_recall(int(trig[i]))))
            run_threads(callers, lambda i: got.__setitem__(("rec", i), co.recommend(qs[i], top_n)))
        finally:
            co.destroy()
        d = serving(ix, s0)
        ix.detach()
    for i in range(callers):
        for name, ref in (("ip", ref_ip), ("l2", ref_l2), ("i2i", ref_i2i)):
            g = got[(name, i)]
            assert g[2] == k
            assert np.array_equal(g[0], ref[0][i]), (name, i)
            assert np.array_equal(bits(g[1]), bits(ref[1][i])), (name, i)
        like_oracle((got[("ip", i)][0][None], got[("ip", i)][1][None]), orow[i:i + 1, :k], osc[i:i + 1, :k])
        like_oracle((got[("l2", i)][0][None], got[("l2", i)][1][None]), lrow[i:i + 1, :k], lsc[i:i + 1, :k])
        g = got[("rec", i)]
        assert g[4] == top_n
        for a, b in zip(g[:4], ref_rec[i]):
            assert np.array_equal(bits(np.asarray(a).reshape(-1)), bits(np.asarray(b).reshape(-1))), i
    assert d["plans_held"] > 0, d
    m.destroy()
    ex.free()


def test_recommend_pipeline_through_the_attached_index(ctx, world):
    t, tab, q, _, _, ix = world
    R, k = 32, 500
    w = o.Dnn3Weights()
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128))
    ex = pa.Expr("${gpu_dnn}*(1+${current_score})^0.1")
    qs = q[100:100 + R]
    ref = pa.recommend_dnn3(ctx, t, m, ex, "gpu_dnn", qs, k)

    def begin_end():
        n = R * k
        d_q = ctx.to_device(np.ascontiguousarray(qs))
        bufs = [ctx.malloc(n * 8), ctx.malloc(n * 4), ctx.malloc(n * 4), ctx.malloc(n * 8), ctx.malloc(n * 4), ctx.malloc(R * 4)]
        tk = C.c_void_p()
        try:
            pa._lib.check(ctx.L.pg_recommend_dnn3_begin(ctx.h, t.h, m.h, ex.h, b"gpu_dnn", d_q, R, k, *bufs, C.byref(tk)))
            pa._lib.check(ctx.L.pg_recommend_end(ctx.h, tk, None))
            outs = [np.zeros((R, k), np.uint64), np.zeros((R, k), np.float32), np.zeros((R, k), np.float32),
                    np.zeros((R, k), np.float64), np.zeros((R, k), np.uint32), np.zeros(R, np.uint32)]
            for a, p in zip(outs, bufs):
                ctx.d2h(a, p)
        finally:
            for p in [d_q] + bufs:
                ctx.free(p)
        return outs

    with wide(ctx):
        ix.attach()
        s0 = serving(ix)
        got_dev = pa.recommend_dnn3(ctx, t, m, ex, "gpu_dnn", qs, k)
        got_be = begin_end()
        d = serving(ix, s0)
        ix.detach()
    for got in (got_dev, got_be):
        for a, b in zip(got, ref):
            assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    assert d["plans"] == 2 and d["plans_held"] == 2, d
    m.destroy()
    ex.free()


def test_stale_index_is_skipped_and_a_new_one_serves(ctx):
    n, d, k = 400_000, 64, 500
    tab = o.synth_mixture_rows(31, 0, n, d, 100, 0.1)
    q = o.synth_mixture_rows(31, 2, 16, d, 100, 0.1, stream=1)
    t = pa.Table(ctx, n, d)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    with wide(ctx):
        ix.attach()
        s0 = serving(ix)
        like_oracle(t.recall_topk(q, k), *o.recall_topk(tab, q, k))
        assert serving(ix, s0)["plans_held"] == 1
        gen = ix.stats()["generation"]
        # new rows: the queries' own vectors land in the table, so the answers change
        tab2 = tab.copy()
        tab2[1000:1016] = q
        t.upload(tab2[1000:1016], row0=1000)
        s1 = serving(ix)
        for l2 in (False, True):
            got = t.recall_topk_l2(q, k) if l2 else t.recall_topk(q, k)
            like_oracle(got, *(o.recall_topk_l2(tab2, q, k) if l2 else o.recall_topk(tab2, q, k)))
        d1 = serving(ix, s1)
        assert d1["skipped_stale"] == 2 and d1["plans"] == 0, d1
        # a new index over the new rows replaces the stale one and serves
        ix2 = pa.Index(ctx, t)
        assert ix2.stats()["generation"] != gen
        ix2.attach()
        s2 = serving(ix2)
        like_oracle(t.recall_topk(q, k), *o.recall_topk(tab2, q, k))
        assert serving(ix2, s2)["plans_held"] == 1
        ix.destroy()                                      # no longer attached: it may go
        ix2.detach()
        ix2.destroy()
    t.destroy()


def test_uniform_table_replans_then_switches_off(ctx):
    n, d, k = 300_000, 128, 1000
    t = pa.Table(ctx, n, d)
    t.fill_synthetic(o.SEED_TABLE)
    tab = o.synth_rows(o.SEED_TABLE, 0, n, d)
    q = o.synth_rows(o.SEED_QUERY, 0, 12, d)
    ref = o.recall_topk(tab, q, k)
    ix = pa.Index(ctx, t)
    with options(ctx, index_skip_batches=(3, 64)):
        ix.attach()
        s0 = serving(ix)
        for i in range(6):                                # one query per batch: band 1
            like_oracle(t.recall_topk(q[i:i + 1], k), ref[0][i:i + 1], ref[1][i:i + 1])
        d1 = serving(ix, s0)
        # tried, dense, three skipped, tried again (dense), one more skipped
        assert d1["replan_dense"] == 2 and d1["plans"] == 2 and d1["plans_held"] == 0, d1
        assert d1["skipped_switch"] == 4, d1
        # another band keeps its own switch
        like_oracle(t.recall_topk(q[:8], k), ref[0][:8], ref[1][:8])
        d2 = serving(ix, s0)
        assert d2["plans"] == 3 and d2["skipped_switch"] == 4, d2
        ix.detach()
    ix.destroy()
    t.destroy()


def test_round_budget_replans_and_several_rounds_hold(ctx):
    """The construction of test_gpu_index.py::test_scan_in_several_rounds: wide lists whose scan needs more than one round of
    2^19 suspects per query."""
    n, d = 3_000_000, 64
    t = pa.Table(ctx, n, d)
    t.fill_synthetic(o.SEED_TABLE)
    tab = o.synth_rows(o.SEED_TABLE, 0, n, d)
    q = o.synth_rows(o.SEED_QUERY, 0, 4, d)
    ix = pa.Index(ctx, t, n_lists=12)
    ref1, ref4 = o.recall_topk(tab, q[:1], 5000), o.recall_topk(tab, q, 3000)
    with wide(ctx), options(ctx, index_plan_rounds=(1, 2), index_skip_batches=(0, 64)):
        ix.attach()
        s0 = serving(ix)
        like_oracle(t.recall_topk(q[:1], 5000), *ref1)
        d1 = serving(ix, s0)
        assert d1["replan_rounds"] == 1 and d1["plans_held"] == 0, d1
        ctx.set_option("index_plan_rounds", 8)
        s1, p1 = serving(ix), ix.stats()
        like_oracle(t.recall_topk(q[:1], 5000), *ref1)
        like_oracle(t.recall_topk(q, 3000), *ref4)
        d2 = serving(ix, s1)
        assert d2["plans_held"] == 2, d2
        assert ix.stats()["max_query_scan_rows"] > 2 ** 19
        assert ix.stats()["pairs_scored"] > p1["pairs_scored"]
        ix.detach()
    ix.destroy()
    t.destroy()


def _hostile_tables(rng):
    """the tables of test_gpu_index.py::test_hostile_data: (table rows, row offset, n_lists values, queries, IP cases, L2 cases),
    a case being (queries, k)"""
    d = 128
    same = np.tile(rng.standard_normal(d).astype(np.float32), (5003, 1))
    q = rng.standard_normal((4, d)).astype(np.float32)
    yield same, 0, (0,), [(q, k) for k in (1, 100, 8000)], [(q, k) for k in (1, 100, 8000)]
    base = rng.integers(-2, 3, size=(3000, d)).astype(np.float32)
    tab = np.concatenate([base, base[::-1], base[:77]]).astype(np.float32)
    onehot = np.zeros((1, d), np.float32)
    onehot[0, 5] = 1
    qs = np.concatenate([np.zeros((1, d), np.float32), onehot, -tab.mean(0, keepdims=True).astype(np.float32),
                         np.float32(1e30) * np.sign(rng.standard_normal((1, d))).astype(np.float32),
                         rng.integers(-1, 2, size=(4, d)).astype(np.float32)]).astype(np.float32)
    yield tab, 1_000_003, (1, tab.shape[0] // 64, 17), [(qs, k) for k in (1, 50, 2000)], [(qs[:3], 300)]
    for dd, nq in ((64, 40), (192, 32), (256, 32)):
        tab = o.synth_mixture_rows(5, 0, 20_011, dd, 20, 0.1)
        q = o.synth_mixture_rows(5, 1, nq, dd, 20, 0.1, stream=1)
        yield tab, 0, (0,), [(q, 700)], ([(q, 700)] if dd == 64 else [])


def _like_oracle_padded(got, ref, l2):
    n = ref[0].shape[1]
    like_oracle((got[0][:, :n], got[1][:, :n]), *ref)
    assert np.asarray(got[2]).tolist() == [n] * got[0].shape[0]
    assert np.all(got[0][:, n:] == np.uint64(0xFFFFFFFFFFFFFFFF))
    assert np.all(got[1][:, n:] == (np.inf if l2 else -np.inf))


def test_hostile_tables_through_the_attached_plan(ctx):
    """test_gpu_index.py's hostile tables through t.recall_topk[_l2] with the index attached (dense rule lifted, a raised round
    budget): bit for bit the detached call and the oracle, and every batch held by the plan.  A table with a NaN / inf row is
    never tried (the plan is not prepared for a non-finite index): the table's plans answer and no counter moves."""
    rng = np.random.default_rng(11)
    for tab, off, n_lists, ip_cases, l2_cases in _hostile_tables(rng):
        t = pa.Table(ctx, tab.shape[0], tab.shape[1], off)
        t.upload(tab)
        cases = [(False, qq, k) for qq, k in ip_cases] + [(True, qq, k) for qq, k in l2_cases]
        detached = [(t.recall_topk_l2 if l2 else t.recall_topk)(qq, k) for l2, qq, k in cases]
        refs = [(o.recall_topk_l2 if l2 else o.recall_topk)(tab, qq, k, row_offset=off) for l2, qq, k in cases]
        for nl in n_lists:
            ix = pa.Index(ctx, t, n_lists=nl)
            with wide(ctx), options(ctx, index_plan_rounds=(8, 2)):
                ix.attach()
                try:
                    for (l2, qq, k), det, ref in zip(cases, detached, refs):
                        s0 = serving(ix)
                        got = (t.recall_topk_l2 if l2 else t.recall_topk)(qq, k)
                        dd = serving(ix, s0)
                        same(got, det)
                        _like_oracle_padded(got, ref, l2)
                        assert dd["plans"] == 1 and dd["plans_held"] == 1 and dd["queries_held"] == qq.shape[0], (tab.shape, nl, l2, k, dd)
                        assert all(dd[c] == 0 for c in ("replan_dense", "replan_rounds", "replan_overflow", "replan_nonfinite",
                                                        "skipped_stale", "skipped_switch")), (tab.shape, nl, l2, k, dd)
                finally:
                    ix.detach()
            ix.destroy()
        if tab.shape[1] > 128:
            # squared Euclidean above dim 128: not routed (no kernel for it), refused by the table as before attaching
            ix = pa.Index(ctx, t)
            with wide(ctx):
                ix.attach()
                s0 = serving(ix)
                with pytest.raises(pa._lib.PgError) as e:
                    t.recall_topk_l2(ip_cases[0][0], 700)
                assert e.value.code == -4
                assert all(v == 0 for v in serving(ix, s0).values())
                ix.detach()
            ix.destroy()
        t.destroy()
    # a NaN / inf row
    tab = o.synth_rows(o.SEED_TABLE, 0, 10_000, 128)
    tab[17, 3] = np.nan
    tab[9000, 0] = np.inf
    t = pa.Table(ctx, tab.shape[0], tab.shape[1])
    t.upload(tab)
    q = o.synth_rows(o.SEED_QUERY, 0, 3, 128)
    det = t.recall_topk(q, 100)
    ix = pa.Index(ctx, t)
    with wide(ctx), options(ctx, index_plan_rounds=(8, 2)):
        ix.attach()
        s0, p0 = serving(ix), ix.stats()
        same(t.recall_topk(q, 100), det)
        assert all(v == 0 for v in serving(ix, s0).values())
        assert ix.stats()["calls"] == p0["calls"]
        ix.detach()
    ix.destroy()
    t.destroy()


def test_edge_cases(ctx, world):
    t, tab, q, (orow, osc), _, ix = world
    k = 100
    # a non-finite query inside a coalesced batch: exact (as the unattached table answers it) and counted
    qs = q[:16].copy()
    qs[5, 3] = np.nan
    ref = [t.recall_topk(qs[i:i + 1], k) for i in range(16)]
    with wide(ctx):
        ix.attach()
        s0 = serving(ix)
        co = pa.Coalescer(ctx, t, k, max_wait_us=3000)
        got = [None] * 16
        try:
            run_threads(16, lambda i: got.__setitem__(i, co.recall(qs[i])))
        finally:
            co.destroy()
        d = serving(ix, s0)
        assert d["replan_nonfinite"] >= 1, d
        for i in range(16):
            assert np.array_equal(got[i][0], ref[i][0][0]) and np.array_equal(bits(got[i][1]), bits(ref[i][1][0])), i
        # a filtered recall is not routed and unchanged
        feats = pa.Features(ctx, N)
        feats.set_column("c", pa.F_I32, np.arange(N, dtype=np.int32) % 3)
        s1, p1 = serving(ix), ix.stats()
        w_att = t.recall_topk_where(feats, "c", "==", 1, q[:8], k)
        # a view of the attached table is not routed
        v = t.view(feats, "c", "==", 1)
        v_att = v.recall_topk(q[:8], k)
        assert serving(ix, s1) == {key: 0 for key in s1} and ix.stats()["calls"] == p1["calls"]
        # refusals: destroy while attached, detach of an index that is not attached, attach of a view's index (none can be built)
        with pytest.raises(pa._lib.PgError) as e:
            ix.destroy()
        assert e.value.code == -1 and ix.h
        # an index of another table: attaching it leaves this table's routing alone
        t2 = pa.Table(ctx, 100_000, D)
        t2.fill_synthetic(o.SEED_TABLE)
        ix2 = pa.Index(ctx, t2)
        with pytest.raises(pa._lib.PgError) as e:
            ix2.detach()
        assert e.value.code == -1
        ix2.attach()
        s2, s22 = serving(ix), serving(ix2)
        same(t.recall_topk(q[:4], k), (orow[:4, :k], osc[:4, :k], np.full(4, k, np.uint32)))
        assert serving(ix, s2)["plans_held"] == 1 and serving(ix2, s22)["plans"] == 0
        ix2.detach()
        ix2.destroy()
        t2.destroy()
        # detach restores the table's pass: the counters stop moving
        ix.detach()
        s3, p3 = serving(ix), ix.stats()
        like_oracle(t.recall_topk(q[:4], k), orow[:4, :k], osc[:4, :k])
        assert serving(ix, s3) == {key: 0 for key in s3} and ix.stats()["calls"] == p3["calls"]
        w_det = t.recall_topk_where(feats, "c", "==", 1, q[:8], k)
        v_det = v.recall_topk(q[:8], k)
    same(w_att, w_det)
    same(v_att, v_det)
    # ... and both equal the oracle on the admitted rows (2 M rows: two scan groups of the filter's block counts)
    ids = np.flatnonzero(np.arange(N) % 3 == 1)
    assert v.rows == ids.size
    frow, fsc = o.recall_topk(tab[ids], q[:8], k)
    frow = ids[frow.astype(np.int64)].astype(np.uint64)
    for got in (w_att, v_att):
        like_oracle(got, frow, fsc)
        assert got[2].tolist() == [k] * 8
    v.destroy()
    feats.destroy()


def test_two_contexts_on_one_attached_index(ctx, world):
    t, tab, q, (orow, osc), _, ix = world
    k = 1000
    ctx2 = pa.Context(0)
    out, errs = {}, []
    with wide(ctx):
        ctx2.set_option("index_dense_fraction", 1e6)
        ix.attach()
        s0 = serving(ix)

        def worker(c, name, sl):
            try:
                for _ in range(3):
                    out[name] = host_recall(c, t, q[sl], k)
            except Exception as e:                    # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=worker, args=(ctx, "a", slice(0, 32))),
              threading.Thread(target=worker, args=(ctx2, "b", slice(32, 64)))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        d = serving(ix, s0)
        ix.detach()
    ctx2.close()
    assert not errs, errs
    like_oracle(out["a"], orow[:32, :k], osc[:32, :k])
    like_oracle(out["b"], orow[32:64, :k], osc[32:64, :k])
    assert d["plans"] == 6 and d["plans_held"] == 6, d
