"""GPU tests of compound WhereClauses (pg_where): the device's bitmap equals pg_where_eval_host word for word;
each recall surface (table, view, index) equals, bit for bit, the existing single-column call on a 0/1 flag column computed in
numpy that admits the same rows, and the CPU oracle over those rows; a one-comparison clause takes the single-column path and
builds nothing; the bitmap and the index's lists follow pg_features_set_column; threads on two contexts share one clause."""
import threading

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
DENSE_DEFAULT = 0.01          # pg_set_option "index_dense_fraction" default
COMPACT_DEFAULT = 8 << 20     # "where_compact_max_rows" default
FALLBACKS = ("fallback_dense", "fallback_stale", "fallback_nonfinite", "fallback_overflow")
BIG = 1 << 40


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_equal_out(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(got[2], want[2])


def unpack(words, n):
    r = np.arange(n)
    return ((words[r >> 5] >> (r & 31).astype(np.uint32)) & 1).astype(bool)


def oracle_where(tab, q, k, mask, l2=False):
    """the oracle over the admitted rows alone, local rows mapped back through np.flatnonzero(mask), padded to k"""
    ids = np.flatnonzero(mask)
    nq = q.shape[0]
    rows = np.full((nq, k), U64MAX, np.uint64)
    sc = np.full((nq, k), np.inf if l2 else -np.inf, np.float32)
    n = min(k, ids.size)
    if n:
        orow, osc = (o.recall_topk_l2 if l2 else o.recall_topk)(tab[ids], q, k)
        rows[:, :n] = ids[orow.astype(np.int64)].astype(np.uint64)
        sc[:, :n] = osc
    return rows, sc, np.full(nq, n, np.uint32)


def check_vs_oracle(got, tab, q, k, mask, l2):
    """counts and padding of every query, ids and score bits of three of them"""
    nq = q.shape[0]
    m = min(k, int(mask.sum()))
    assert got[2].tolist() == [m] * nq
    assert np.all(got[0][:, m:] == U64MAX)
    sel = sorted({0, nq // 2, nq - 1})
    ref = oracle_where(tab, q[sel], k, mask, l2)
    assert np.array_equal(got[0][sel], ref[0])
    assert np.array_equal(bits(got[1][sel]), bits(ref[1]))


class Store:
    """a feature store and its host copy: 16 columns c0 .. c15 (even: int32, odd: int64 beyond 2^40) of small values, ts (uniform
    0 .. 999 999, int32), ts64, and a flag column the baseline calls filter on"""

    def __init__(self, ctx, n, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        self.cols = {}
        for i in range(16):
            v = rng.integers(0, 8 + i, n)
            self.cols["c%d" % i] = (BIG + v).astype(np.int64) if i % 2 else v.astype(np.int32)
        self.cols["ts"] = rng.integers(0, 1_000_000, n).astype(np.int32)
        self.cols["ts64"] = BIG + rng.integers(0, 1_000_000, n).astype(np.int64)
        self.feats = pa.Features(ctx, n)
        for name, v in self.cols.items():
            self.set(name, v)
        self.feats.set_column("f", pa.F_F32, np.zeros(n, np.float32))

    def set(self, name, v):
        self.cols[name] = v
        self.feats.set_column(name, pa.F_I64 if v.dtype == np.int64 else pa.F_I32, v)

    def mask(self, np_mask):
        """the admitted rows of a case, computed in numpy from the host columns: a reference the compiler has no part in"""
        m = np_mask(self.cols)
        assert m.dtype == np.bool_ and m.shape == (self.n,)
        return m

    def set_flag(self, mask):
        self.feats.set_column("flag", pa.F_I32, mask.astype(np.int32))


class options:
    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, (v, _) in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *a):
        for k, (_, d) in self.kv.items():
            self.ctx.set_option(k, d)


N, D, K = 900_000, 128, 500


@pytest.fixture(scope="module")
def world(ctx):
    rng = np.random.default_rng(71)
    tab = o.synth_rows(o.SEED_TABLE, 0, N, D) * rng.uniform(0.7, 1.3, (N, 1)).astype(np.float32)
    t = pa.Table(ctx, N, D)
    t.upload(tab)
    st = Store(ctx, N, 0xC0DE)
    yield tab, t, st
    st.feats.destroy()
    t.destroy()


def queries(nq):
    return (o.synth_rows(o.SEED_QUERY, 11 * nq, nq, D) * np.float32(1.1)).astype(np.float32)


IN_1024 = ",".join(str(v) for v in np.random.default_rng(4).permutation(8192)[:1024] * 122)
BITS_CLAUSES = [
    "ts > 500000 AND c0 = 1",
    "c1 >= %d" % (BIG + 3) + " OR NOT c2 IN (0, 5, 2)",
    "ts64 BETWEEN %d AND %d AND ts NOT BETWEEN 1000 AND 900000" % (BIG + 100_000, BIG + 800_000),
    "ts IN (%s)" % IN_1024,
    "ts64 NOT IN (%s) AND c3 <> %d" % (",".join(str(BIG + int(v)) for v in range(0, 1_000_000, 1999)), BIG + 1),
    " AND ".join("c%d %s %d" % (i, (">=", "<", "!=", "<=")[i % 4], (BIG if i % 2 else 0) + 1 + i % 5) for i in range(16)),
    " OR ".join("(c%d = %d AND c%d > %d)" % (i, (BIG if i % 2 else 0) + i % 3, (i + 7) % 16, (BIG if (i + 7) % 2 else 0) + 2) for i in range(16)),
    "NOT ((c0 < 3 OR c5 = %d) AND NOT (ts < 250000 OR (c8 IN (1,2,3) AND c9 > %d)))" % (BIG + 2, BIG + 4),
    "ts > 500000",                    # (a plain comparison has a bitmap too when pg_where_bits asks for it)
    "ts < 0 AND c0 = 1",              # nothing passes
    "ts >= 0 OR c0 = 1",              # everything passes
]


_E = lambda i: BIG if i % 2 else 0                 # (odd columns are int64 beyond 2^40)
_CMP = {">=": np.greater_equal, "<": np.less, "!=": np.not_equal, "<=": np.less_equal}
BITS_NUMPY = {      # the 16-column clauses and the NOT-nest in numpy: the host evaluation itself is pinned on them here
    BITS_CLAUSES[5]: lambda c: np.logical_and.reduce([_CMP[(">=", "<", "!=", "<=")[i % 4]](c["c%d" % i], _E(i) + 1 + i % 5) for i in range(16)]),
    BITS_CLAUSES[6]: lambda c: np.logical_or.reduce([(c["c%d" % i] == _E(i) + i % 3) & (c["c%d" % ((i + 7) % 16)] > _E(i + 7) + 2)
                                                     for i in range(16)]),
    BITS_CLAUSES[7]: lambda c: ~(((c["c0"] < 3) | (c["c5"] == BIG + 2)) &
                                 ~((c["ts"] < 250000) | (np.isin(c["c8"], [1, 2, 3]) & (c["c9"] > BIG + 4)))),
    BITS_CLAUSES[3]: lambda c: np.isin(c["ts"], [int(v) for v in IN_1024.split(",")]),
}


@pytest.mark.parametrize("rows", [N, N - 13, 1000, 31])
def test_device_bitmap_equals_host_evaluation(ctx, world, rows):
    """pg_where_bits == pg_where_eval_host, word for word and in the count, at 900 000 rows and at row counts that are no
    multiple of 32 or 1024; 1 to 16 columns of both dtypes, an IN list of 1024 constants"""
    _, _, st = world
    assert rows % 32 or rows == N
    for clause in BITS_CLAUSES:
        w = pa.Where(clause)
        host = w.eval_host({c: st.cols[c][:rows] for c in w.columns}, rows)
        if clause in BITS_NUMPY:
            assert np.array_equal(unpack(host, rows), BITS_NUMPY[clause](st.cols)[:rows]), clause
        dev, admitted = w.bits(ctx, st.feats, rows)
        assert np.array_equal(dev, host), clause
        assert admitted == int(unpack(host, rows).sum()), clause
        s = w.stats()
        assert s["builds"] == 1 and s["admitted"] == admitted and s["bytes"] >= rows // 8
        dev2, _ = w.bits(ctx, st.feats, rows)                                  # from the cache
        assert np.array_equal(dev2, host) and w.stats()["builds"] == 1 and w.stats()["hits"] == 1
        w.free()


def test_binding_refusals(ctx, world):
    _, t, st = world
    q = queries(1)
    for clause, what in (("nope = 1 AND ts > 0", "no column"), ("f > 0 AND ts > 0", "int32 / int64")):
        w = pa.Where(clause)
        with pytest.raises(pa._lib.PgError) as e:
            t.recall_topk_where_ex(st.feats, w, q, K)
        assert e.value.code == -1 and what in str(e.value)
        with pytest.raises(pa._lib.PgError) as e:
            t.view_where(st.feats, w)
        assert e.value.code == -1
        w.free()
    w = pa.Where("ts > 0 AND c0 = 1")
    small = pa.Features(ctx, 1000)
    small.set_column("ts", pa.F_I32, np.zeros(1000, np.int32))
    small.set_column("c0", pa.F_I32, np.zeros(1000, np.int32))
    with pytest.raises(pa._lib.PgError) as e:
        t.recall_topk_where_ex(small, w, q, K)
    assert e.value.code == -1 and "rows" in str(e.value)
    with pytest.raises(pa._lib.PgError) as e:
        t.recall_topk_where_ex(st.feats, w, q, 0)
    assert e.value.code == -4                                                  # k: PG_ERR_UNSUPPORTED, as pg_recall_topk_where
    small.destroy()
    w.free()


# selectivities from one row in two to fewer rows than K and none; both metrics; 1, 3, 40, 130, 200, 256 queries
RECALL_CASES = [
    ("ts > 500000 OR c0 = 1 AND c1 = %d" % (BIG + 1), lambda c: (c["ts"] > 500000) | ((c["c0"] == 1) & (c["c1"] == BIG + 1)), 40, False),   # ~ one in two
    ("ts >= 800000 AND c2 <> 3", lambda c: (c["ts"] >= 800000) & (c["c2"] != 3), 200, False),                                             # ~ one in six
    ("ts >= 800000 AND c2 IN (0, 1, 2, 3, 4)", lambda c: (c["ts"] >= 800000) & np.isin(c["c2"], [0, 1, 2, 3, 4]), 256, False),            # ~ one in ten
    ("ts < 10000 AND NOT c4 = 0", lambda c: (c["ts"] < 10000) & ~(c["c4"] == 0), 3, False),                                               # ~ one in a hundred
    ("ts BETWEEN 100 AND 700 AND c0 IN (1, 2)", lambda c: (c["ts"] >= 100) & (c["ts"] <= 700) & np.isin(c["c0"], [1, 2]), 1, False),      # fewer rows than K
    ("ts64 > %d AND (c3 = %d OR c5 = %d)" % (BIG + 700_000, BIG + 2, BIG + 4),
     lambda c: (c["ts64"] > BIG + 700_000) & ((c["c3"] == BIG + 2) | (c["c5"] == BIG + 4)), 130, False),
    ("ts > 500000 AND NOT (c0 = 1 AND c1 = %d)" % (BIG + 1), lambda c: (c["ts"] > 500000) & ~((c["c0"] == 1) & (c["c1"] == BIG + 1)), 40, True),   # squared Euclidean
    ("ts >= 900000 AND c6 < 12", lambda c: (c["ts"] >= 900000) & (c["c6"] < 12), 130, True),
    ("ts64 < %d OR ts IN (5, 6, 7)" % (BIG + 200), lambda c: (c["ts64"] < BIG + 200) | np.isin(c["ts"], [5, 6, 7]), 1, True),             # fewer rows than K
    ("ts >= 990000 AND c2 IN (1, 2)", lambda c: (c["ts"] >= 990000) & np.isin(c["c2"], [1, 2]), 256, True),
    ("ts < 0 AND c0 = 1", lambda c: (c["ts"] < 0) & (c["c0"] == 1), 3, False),                                                            # nothing passes
    ("ts > 2000000 OR c0 > 100", lambda c: (c["ts"] > 2000000) | (c["c0"] > 100), 1, True),
]


@pytest.mark.parametrize("compact_max", [0, COMPACT_DEFAULT])
def test_table_recall_equals_flag_column_and_oracle(ctx, world, compact_max):
    """pg_recall_topk_where_ex == pg_recall_topk_where on a flag column admitting the same rows, bit for bit, and == the oracle on
    the admitted rows; with "where_compact_max_rows" 0 (every filter in place) and at its default (selective ones compacted)"""
    tab, t, st = world
    with options(ctx, where_compact_max_rows=(compact_max, COMPACT_DEFAULT)):
        for clause, np_mask, nq, l2 in RECALL_CASES:
            w = pa.Where(clause)
            mask = st.mask(np_mask)
            st.set_flag(mask)
            q = queries(nq)
            base = t.recall_topk_where(st.feats, "flag", "==", 1, q, K, l2=l2)
            got = t.recall_topk_where_ex(st.feats, w, q, K, l2=l2)
            assert_equal_out(got, base)
            check_vs_oracle(got, tab, q, K, mask, l2)
            assert_equal_out(t.recall_topk_where_ex(st.feats, w, q, K, l2=l2), base)       # the cached bitmap
            s = w.stats()
            assert s["builds"] == 1 and s["hits"] == 1 and s["admitted"] == int(mask.sum()), (clause, s)
            w.free()


def test_one_comparison_takes_the_single_column_path_and_builds_nothing(ctx, world):
    _, t, st = world
    for clause, col, op, v, nq, l2 in (("ts > 500000", "ts", ">", 500000, 40, False), ("NOT (ts64 >= %d)" % (BIG + 900), "ts64", "<", BIG + 900, 3, True),
                                       ("((c1 <> %d))" % (BIG + 2), "c1", "!=", BIG + 2, 130, False)):
        w = pa.Where(clause)
        q = queries(nq)
        assert_equal_out(t.recall_topk_where_ex(st.feats, w, q, K, l2=l2), t.recall_topk_where(st.feats, col, op, v, q, K, l2=l2))
        s = w.stats()
        assert s["builds"] == 0 and s["hits"] == 0 and s["bytes"] == 0, s
        w.free()


def test_view_of_a_compound_clause(ctx, world):
    tab, t, st = world
    for clause, np_mask in (("ts >= 800000 AND c2 IN (0, 1, 2, 3, 4)", lambda c: (c["ts"] >= 800000) & np.isin(c["c2"], [0, 1, 2, 3, 4])),
                            ("ts < 3000 OR c0 = 1 AND ts64 > %d" % (BIG + 990_000),
                             lambda c: (c["ts"] < 3000) | ((c["c0"] == 1) & (c["ts64"] > BIG + 990_000)))):
        w = pa.Where(clause)
        mask = st.mask(np_mask)
        st.set_flag(mask)
        v = t.view_where(st.feats, w)
        vb = t.view(st.feats, "flag", "==", 1)
        assert v.rows == int(mask.sum()) == vb.rows == w.stats()["admitted"]
        for nq, l2 in ((3, False), (40, True)):
            q = queries(nq)
            got = (v.recall_topk_l2 if l2 else v.recall_topk)(q, K)
            assert_equal_out(got, (vb.recall_topk_l2 if l2 else vb.recall_topk)(q, K))
            check_vs_oracle(got, tab, q, K, mask, l2)                          # source row ids
        v.destroy()
        vb.destroy()
        w.free()
    w = pa.Where("ts < 0 AND c0 = 1")
    with pytest.raises(pa._lib.PgError) as e:
        t.view_where(st.feats, w)
    assert e.value.code == -8                                                  # PG_ERR_EMPTY, as pg_table_view_create
    w.free()


# ---- through the index ----------------------------------------------------------------------------------------------------
NI, DI, CENTRES, SIGMA, SEED = 600_000, 64, 100, 0.1, 0x3E0064        # the dim-64 world of tests/test_gpu_index_where.py


@pytest.fixture(scope="module")
def iworld(ctx):
    tab = o.synth_mixture_rows(SEED, 0, NI, DI, CENTRES, SIGMA)
    q = o.synth_mixture_rows(SEED, 991, 256, DI, CENTRES, SIGMA, stream=1)
    t = pa.Table(ctx, NI, DI)
    t.fill_mixture(SEED, CENTRES, SIGMA)
    ix = pa.Index(ctx, t)
    r = ix.read()
    cl = np.empty(NI, np.int32)
    for L in range(len(r["offsets"]) - 1):
        cl[r["perm"][r["offsets"][L]:r["offsets"][L + 1]]] = L
    st = Store(ctx, NI, SEED)
    st.set("cl10", cl % 10)
    st.set("u", np.random.default_rng(SEED).integers(0, 1000, NI).astype(np.int32))
    yield tab, q, t, ix, st
    st.feats.destroy()
    ix.destroy()
    t.destroy()


def stats_delta(ix, before):
    after = ix.stats()
    return {k: after[k] - before[k] for k in ("calls", "queries") + FALLBACKS}


def lists_delta(ix, before):
    after = ix.where_stats()
    return {k: after[k] - before[k] for k in ("builds", "hits")}


INDEX_CASES = [
    ("u < 300 AND cl10 IN (1, 4, 7)", lambda c: (c["u"] < 300) & np.isin(c["cl10"], [1, 4, 7]), 8, 300, False),        # ~ one in eleven, correlated with the lists
    ("u < 100 OR (cl10 = 3 AND c0 = 1)", lambda c: (c["u"] < 100) | ((c["cl10"] == 3) & (c["c0"] == 1)), 40, 500, False),
    ("ts64 >= %d AND NOT cl10 BETWEEN 2 AND 8" % (BIG + 500_000),
     lambda c: (c["ts64"] >= BIG + 500_000) & ~((c["cl10"] >= 2) & (c["cl10"] <= 8)), 1, 300, True),
    ("u < 2 AND c1 = %d" % (BIG + 1), lambda c: (c["u"] < 2) & (c["c1"] == BIG + 1), 130, 500, True),                  # fewer rows than K
    ("u < 0 AND cl10 = 1", lambda c: (c["u"] < 0) & (c["cl10"] == 1), 3, 100, False),                                  # nothing passes
    ("u >= 500 OR cl10 < 5", lambda c: (c["u"] >= 500) | (c["cl10"] < 5), 256, 200, False),                            # three rows in four
]
U_CL = lambda c: (c["u"] < 300) & np.isin(c["cl10"], [1, 4, 7])


def test_index_recall_equals_table_recall_and_falls_back_only_where_the_flag_column_does(ctx, iworld):
    tab, qs, t, ix, st = iworld
    for lifted in (True, False):
        # lifted: the dense rule (a cost decision calibrated at 100 M rows) out of the way, so the index's search serves the
        # flag-column baseline; default: whatever the baseline does, the compound call does the same
        with options(ctx, index_dense_fraction=(1e6 if lifted else DENSE_DEFAULT, DENSE_DEFAULT)):
            for clause, np_mask, nq, k, l2 in INDEX_CASES:
                w = pa.Where(clause)
                mask = st.mask(np_mask)
                st.set_flag(mask)
                q = qs[:nq]
                b = ix.stats()
                base = ix.recall_topk_where(st.feats, "flag", "==", 1, q, k, l2=l2)
                d_base = stats_delta(ix, b)
                if lifted:
                    assert all(d_base[f] == 0 for f in FALLBACKS), (clause, d_base)      # the baseline is served by the index
                b, lb = ix.stats(), ix.where_stats()
                got = ix.recall_topk_where_ex(st.feats, w, q, k, l2=l2)
                assert stats_delta(ix, b) == d_base, (clause, stats_delta(ix, b), d_base)
                assert lists_delta(ix, lb) == {"builds": 1, "hits": 0}, clause
                assert_equal_out(got, base)
                assert_equal_out(got, t.recall_topk_where_ex(st.feats, w, q, k, l2=l2))
                check_vs_oracle(got, tab, q, k, mask, l2)
                b, lb = ix.stats(), ix.where_stats()
                assert_equal_out(ix.recall_topk_where_ex(st.feats, w, q, k, l2=l2), base)  # the second call: the lists' cache
                assert stats_delta(ix, b) == d_base
                assert lists_delta(ix, lb) == {"builds": 0, "hits": 1}, clause
                assert w.stats()["builds"] == 1
                w.free()


def test_a_rewritten_column_rebuilds_the_bitmap_and_the_lists(ctx, iworld):
    tab, qs, t, ix, st = iworld
    q, k = qs[:16], 300
    w = pa.Where("u < 300 AND cl10 IN (1, 4, 7)")
    old_u = st.cols["u"]
    try:
        with options(ctx, index_dense_fraction=(1e6, DENSE_DEFAULT)):
            m0 = st.mask(U_CL)
            check_vs_oracle(ix.recall_topk_where_ex(st.feats, w, q, k), tab, q, k, m0, False)
            e0 = w.stats()["epoch"]
            st.set("c0", st.cols["c0"].copy())                                # a column the clause does not read: nothing rebuilt
            lb = ix.where_stats()
            ix.recall_topk_where_ex(st.feats, w, q, k)
            assert w.stats()["builds"] == 1 and w.stats()["epoch"] == e0 and lists_delta(ix, lb) == {"builds": 0, "hits": 1}
            st.set("u", (999 - old_u).astype(np.int32))
            m1 = st.mask(U_CL)
            assert not np.array_equal(m0, m1)
            lb = ix.where_stats()
            got = ix.recall_topk_where_ex(st.feats, w, q, k)
            s = w.stats()
            assert s["builds"] == 2 and s["epoch"] != e0 and s["admitted"] == int(m1.sum()), s
            assert lists_delta(ix, lb) == {"builds": 1, "hits": 0}
            check_vs_oracle(got, tab, q, k, m1, False)
            check_vs_oracle(t.recall_topk_where_ex(st.feats, w, q, k), tab, q, k, m1, False)
            assert w.stats()["builds"] == 2
    finally:
        st.set("u", old_u)
        w.free()


def test_plain_ex_call_routes_through_an_attached_index(ctx, iworld):
    tab, qs, t, ix, st = iworld
    q, k = qs[:8], 300
    w = pa.Where("u < 300 AND cl10 IN (1, 4, 7)")
    ref = t.recall_topk_where_ex(st.feats, w, q, k)
    ix.attach()
    try:
        with options(ctx, index_dense_fraction=(1e6, DENSE_DEFAULT)):
            b = ix.stats()
            assert_equal_out(t.recall_topk_where_ex(st.feats, w, q, k), ref)
            assert stats_delta(ix, b)["calls"] == 0                            # the default: not routed
            with options(ctx, index_route_where=(1, 0)):
                b = ix.stats()
                assert_equal_out(t.recall_topk_where_ex(st.feats, w, q, k), ref)
                d = stats_delta(ix, b)
                assert d["calls"] == 1 and d["queries"] == 8 and all(d[f] == 0 for f in FALLBACKS), d
    finally:
        ix.detach()
        w.free()


def test_eight_threads_on_two_contexts_share_one_clause(ctx, world):
    tab, t, st = world
    w = pa.Where("ts >= 800000 AND c2 IN (0, 1, 2, 3, 4)")
    q = queries(16)
    ctx2 = pa.Context(0)
    old_ts = st.cols["ts"]

    def run_all():
        out, errs = [None] * 8, []

        def worker(i, c):
            try:
                for _ in range(3):
                    out[i] = w._recall(c, c.L.pg_recall_topk_where_ex, t.h, D, st.feats, q, K, False)
            except BaseException as e:                # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=worker, args=(i, (ctx, ctx2)[i % 2])) for i in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        return out

    try:
        out = run_all()
        np_mask = lambda c: (c["ts"] >= 800000) & np.isin(c["c2"], [0, 1, 2, 3, 4])
        check_vs_oracle(out[0], tab, q, K, st.mask(np_mask), False)
        for r in out[1:]:
            assert_equal_out(r, out[0])
        s = w.stats()
        assert s["builds"] == 1 and s["hits"] == 23, s                        # one build per column version
        st.set("ts", (999_999 - old_ts).astype(np.int32))
        out = run_all()
        check_vs_oracle(out[0], tab, q, K, st.mask(np_mask), False)
        for r in out[1:]:
            assert_equal_out(r, out[0])
        s = w.stats()
        assert s["builds"] == 2 and s["hits"] == 46, s
    finally:
        st.set("ts", old_ts)
        ctx2.close()
        w.free()
