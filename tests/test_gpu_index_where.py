"""GPU tests of the filtered recall through an exact index (pg_index_recall_topk_where): every call equals
pg_recall_topk_where on the same table (ids, order, score bits, counts) and the CPU oracle over the admitted rows; the filtered
lists equal a stable filter of the index's lists; the cache follows every change of the filter, the column and the table; the
fallbacks stay exact and are counted; two contexts share one index; and pg_recall_topk_where routes through an attached index
when asked to."""
import threading

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

DENSE_DEFAULT = 0.01          # pg_set_option "index_dense_fraction" default
CACHE_DEFAULT = 4             # "index_where_cache" default
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
OPS = {">": 0, ">=": 1, "<": 2, "<=": 3, "==": 4, "!=": 5}
NP_OPS = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal, "==": np.equal, "!=": np.not_equal}
FALLBACKS = ("fallback_dense", "fallback_stale", "fallback_nonfinite", "fallback_overflow")
BIG = 1 << 33                 # int64 column values beyond 2^31


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_equal_out(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(got[2], want[2])


def oracle_where(tab, q, k, mask, l2=False, row_offset=0):
    """the oracle over the admitted rows (tab[mask]), local rows mapped back through np.flatnonzero(mask), padded to k"""
    ids = np.flatnonzero(mask)
    nq = q.shape[0]
    rows = np.full((nq, k), U64MAX, np.uint64)
    sc = np.full((nq, k), np.inf if l2 else -np.inf, np.float32)
    n = min(k, ids.size)
    if n:
        orow, osc = (o.recall_topk_l2 if l2 else o.recall_topk)(tab[ids], q, k)
        assert orow.shape[1] == n
        rows[:, :n] = ids[orow.astype(np.int64)].astype(np.uint64) + np.uint64(row_offset)
        sc[:, :n] = osc
    return rows, sc, np.full(nq, n, np.uint32)


def delta(ix, before):
    after = ix.stats()
    return {k: after[k] - before[k] for k in ("calls", "queries", "pairs_scored", "rows_scored", "rows_live") + FALLBACKS}


def where_delta(ix, before):
    after = ix.where_stats()
    return {k: after[k] - before[k] for k in ("builds", "hits", "evictions")}


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


def lifted(ctx):
    # the dense rule is a cost decision calibrated at 100 M rows: lifted so that the search itself serves
    return options(ctx, index_dense_fraction=(1e6, DENSE_DEFAULT))


class World:
    """a clustered table, its index and a feature store: u (uniform 0..999), big (int64 beyond 2^31), cl10 (the row's list id
    mod 10: correlated with the clusters), anti (1 for the rows nearest the queries: an anti-correlated filter admits anti == 0)"""

    def __init__(self, ctx, n, d, centres, sigma, seed, row_offset=0):
        self.tab = o.synth_mixture_rows(seed, 0, n, d, centres, sigma)
        self.q = o.synth_mixture_rows(seed, 991, 256, d, centres, sigma, stream=1)
        self.t = pa.Table(ctx, n, d, row_offset)
        if row_offset or d not in (64, 128):        # (fill_mixture: dim 64 / 128)
            self.t.upload(self.tab)
        else:
            self.t.fill_mixture(seed, centres, sigma)
        self.row_offset = row_offset
        self.ix = pa.Index(ctx, self.t)
        rng = np.random.default_rng(seed)
        r = self.ix.read()
        cl = np.empty(n, np.int32)
        for L in range(len(r["offsets"]) - 1):
            cl[r["perm"][r["offsets"][L]:r["offsets"][L + 1]]] = L
        near = np.unique(o.recall_topk(self.tab, self.q[:8], 2000)[0].astype(np.int64))
        anti = np.zeros(n, np.int32)
        anti[near] = 1
        self.cols = {"u": rng.integers(0, 1000, n).astype(np.int32), "cl10": cl % 10, "anti": anti}
        self.cols["big"] = BIG + self.cols["u"].astype(np.int64) * 7919
        self.feats = pa.Features(ctx, n)
        for name, v in self.cols.items():
            self.feats.set_column(name, pa.F_I64 if v.dtype == np.int64 else pa.F_I32, v)
        self.feats.set_column("f", pa.F_F32, np.zeros(n, np.float32))

    def mask(self, col, op, value):
        return NP_OPS[op](self.cols[col], value)

    def destroy(self):
        self.feats.destroy()
        self.ix.destroy()
        self.t.destroy()


@pytest.fixture(scope="module")
def w64(ctx):
    w = World(ctx, 600_000, 64, 100, 0.1, 0x3E0064)
    yield w
    w.destroy()


@pytest.fixture(scope="module")
def w128(ctx):
    w = World(ctx, 1_000_000, 128, 200, 0.1, 0x3E0128)
    yield w
    w.destroy()


def check_case(ctx, w, col, op, value, nq, k, l2=False):
    """one filter under the default dense rule and with it lifted: equal to Table.recall_topk_where and to the oracle both times,
    and with the rule lifted answered by the search (no fallback)"""
    q = w.q[:nq]
    mask = w.mask(col, op, value)
    ref = oracle_where(w.tab, q, k, mask, l2, w.row_offset)
    table = w.t.recall_topk_where(w.feats, col, op, value, q, k, l2=l2)
    assert_equal_out(table, ref)
    assert_equal_out(w.ix.recall_topk_where(w.feats, col, op, value, q, k, l2=l2), ref)
    b = w.ix.stats()
    with lifted(ctx):
        assert_equal_out(w.ix.recall_topk_where(w.feats, col, op, value, q, k, l2=l2), ref)
    d = delta(w.ix, b)
    assert d["calls"] == 1 and d["queries"] == nq and all(d[f] == 0 for f in FALLBACKS), (col, op, value, d)
    if mask.any():
        assert d["pairs_scored"] > 0, d
        assert d["pairs_scored"] <= int(mask.sum()) * nq, d
    else:
        assert d["pairs_scored"] == 0, d
    return mask


# (column, op, value, nq, k, l2): every op on both column types, selectivities 50 / 10 / 1 %, fewer than K and no admitted row,
# correlated and anti-correlated filters, both metrics, nq in {1, 8, 64, 256}, k in {1, 100, 5000}
CASES = [
    ("u", "<", 500, 8, 5000, False),          # 50 %
    ("u", "<", 100, 64, 100, False),          # 10 %
    ("u", "<", 100, 8, 5000, True),
    ("u", "<", 10, 256, 100, False),          # 1 %
    ("u", "<", 10, 1, 5000, True),
    ("u", ">", 899, 1, 1, False),
    ("u", ">=", 900, 64, 100, True),
    ("u", "<=", 99, 256, 1, False),
    ("u", "==", 7, 8, 5000, False),           # ~0.1 %: fewer than K admitted
    ("u", "!=", 7, 1, 100, False),
    ("u", ">", 5000, 8, 100, False),          # none admitted
    ("u", ">", 5000, 1, 5000, True),
    ("big", ">", BIG + 900 * 7919, 8, 100, False),
    ("big", ">=", BIG + 990 * 7919, 1, 5000, False),
    ("big", "<", BIG + 100 * 7919, 64, 100, True),
    ("big", "<=", BIG + 9 * 7919, 8, 1, False),
    ("big", "==", BIG + 500 * 7919, 256, 100, False),
    ("big", "!=", BIG + 500 * 7919, 1, 100, True),
    ("cl10", "==", 3, 8, 5000, False),        # correlated with the clusters
    ("cl10", "==", 3, 64, 100, True),
    ("anti", "==", 0, 8, 5000, False),        # the rows nearest the queries rejected
    ("anti", "==", 0, 1, 1, True),
]


@pytest.mark.parametrize("case", CASES, ids=["%s%s%d-nq%d-k%d%s" % (c[0], c[1], c[2] - (BIG if c[0] == "big" else 0), c[3], c[4],
                                                                        "-l2" if c[5] else "") for c in CASES])
def test_exact_dim64(ctx, w64, case):
    check_case(ctx, w64, *case)


@pytest.mark.parametrize("case", CASES, ids=["%s%s%d-nq%d-k%d%s" % (c[0], c[1], c[2] - (BIG if c[0] == "big" else 0), c[3], c[4],
                                                                        "-l2" if c[5] else "") for c in CASES])
def test_exact_dim128(ctx, w128, case):
    check_case(ctx, w128, *case)


def test_exact_dim256_inner_product(ctx):
    w = World(ctx, 200_000, 256, 50, 0.1, 0x3E0256)
    try:
        for col, op, value, nq, k in (("u", "<", 100, 32, 100), ("u", "<", 10, 1, 5000), ("u", "==", 3, 8, 5000),
                                      ("big", ">=", BIG + 500 * 7919, 32, 1), ("cl10", "==", 3, 8, 100), ("anti", "==", 0, 32, 5000)):
            check_case(ctx, w, col, op, value, nq, k)
        # at most 32 queries at dim > 128: the same refusal as pg_recall_topk_where
        for fn in (w.t.recall_topk_where, w.ix.recall_topk_where):
            with pytest.raises(pa._lib.PgError) as e:
                fn(w.feats, "u", "<", 100, w.q[:33], 100)
            assert e.value.code == -1
    finally:
        w.destroy()


def test_exact_row_offset(ctx):
    w = World(ctx, 300_000, 128, 60, 0.1, 0x3E0F5E, row_offset=7_000_000)
    try:
        for col, op, value, nq, k, l2 in (("u", "<", 100, 8, 1000, False), ("u", "<", 10, 64, 100, True), ("u", "==", 5, 1, 5000, False),
                                          ("cl10", "!=", 3, 8, 100, True)):
            check_case(ctx, w, col, op, value, nq, k, l2)
    finally:
        w.destroy()


def test_pruning_is_real(ctx, w128):
    """a 10 % random filter on a clustered table, the dense rule lifted: no fallback, and the pairs scored are a small part of
    the admitted rows x queries"""
    mask = w128.mask("u", "<", 100)
    adm = int(mask.sum())
    for nq in (1, 8):
        q = w128.q[:nq]
        b = w128.ix.stats()
        with lifted(ctx):
            got = w128.ix.recall_topk_where(w128.feats, "u", "<", 100, q, 1000)
        d = delta(w128.ix, b)
        assert_equal_out(got, oracle_where(w128.tab, q, 1000, mask))
        assert all(d[f] == 0 for f in FALLBACKS), d
        assert 1000 * nq <= d["pairs_scored"] <= 0.2 * adm * nq, (nq, adm, d)


def test_where_read_is_a_stable_filter(ctx, w64):
    r = w64.ix.read()
    perm, off = r["perm"].astype(np.int64), r["offsets"].astype(np.int64)
    for col, op, value in (("u", "<", 100), ("big", "==", BIG + 3 * 7919), ("cl10", "==", 3), ("anti", "==", 0), ("u", ">", 5000)):
        keep = w64.mask(col, op, value)[perm]
        cum = np.concatenate([[0], np.cumsum(keep)])
        got = w64.ix.where_read(w64.feats, col, op, value)
        assert got["admitted"] == int(keep.sum())
        assert np.array_equal(got["offsets"], cum[off].astype(np.uint32))
        for L in range(len(off) - 1):           # list by list: the index's rows of L that pass, in the index's order
            seg = perm[off[L]:off[L + 1]]
            assert np.array_equal(got["perm"][cum[off[L]]:cum[off[L + 1]]], seg[keep[off[L]:off[L + 1]]]), (col, L)
        assert np.array_equal(got["perm"], perm[keep].astype(np.uint32))


def test_cache(ctx, w64):
    w = w64
    q, k = w.q[:8], 200
    ix, feats = w.ix, w.feats

    def same_as_table(col, op, value):
        got = ix.recall_topk_where(feats, col, op, value, q, k)
        assert_equal_out(got, w.t.recall_topk_where(feats, col, op, value, q, k))
        return got

    with lifted(ctx):
        same_as_table("u", "<", 250)
        b = ix.where_stats()
        same_as_table("u", "<", 250)                                   # a repeated filter is a hit
        assert where_delta(ix, b) == {"builds": 0, "hits": 1, "evictions": 0}
        for col, op, value in (("u", "<", 251), ("u", "<=", 250), ("cl10", "<", 250)):   # value, op, column: new lists
            b = ix.where_stats()
            same_as_table(col, op, value)
            assert where_delta(ix, b)["builds"] == 1, (col, op, value)
        # a set_column on the filtered column: the same pointer, new values — the cached lists must not serve it
        rng = np.random.default_rng(5)
        v1 = rng.integers(0, 1000, w.tab.shape[0]).astype(np.int32)
        feats.set_column("u2", pa.F_I32, v1)
        first = same_as_table("u2", "<", 100)
        assert_equal_out(first, oracle_where(w.tab, q, k, v1 < 100))
        v2 = rng.integers(0, 1000, w.tab.shape[0]).astype(np.int32)
        b = ix.where_stats()
        feats.set_column("u2", pa.F_I32, v2)
        got = same_as_table("u2", "<", 100)
        assert where_delta(ix, b)["builds"] == 1
        assert_equal_out(got, oracle_where(w.tab, q, k, v2 < 100))
        assert not np.array_equal(got[0], first[0])
        st = ix.where_stats()
        assert st["entries"] == CACHE_DEFAULT and st["bytes"] > 0
        # one entry: every new filter evicts; 0: built per call, nothing held
        with options(ctx, index_where_cache=(1, CACHE_DEFAULT)):
            b = ix.where_stats()
            same_as_table("u", "<", 10)
            same_as_table("u", "<", 20)
            d = where_delta(ix, b)
            assert d["builds"] == 2 and d["evictions"] >= CACHE_DEFAULT, d
            st = ix.where_stats()
            adm = int(w.mask("u", "<", 20).sum())
            assert st["entries"] == 1 and st["bytes"] == adm * 4 + (ix.stats()["n_lists"] + 1) * 4, st
        with options(ctx, index_where_cache=(0, CACHE_DEFAULT)):
            b = ix.where_stats()
            same_as_table("u", "<", 30)
            same_as_table("u", "<", 30)
            assert where_delta(ix, b)["builds"] == 2
            assert ix.where_stats()["entries"] == 0 and ix.where_stats()["bytes"] == 0


def test_upload_and_fallbacks(ctx):
    n, d = 200_000, 64
    tab = o.synth_mixture_rows(77, 0, n, d, 40, 0.1)
    q = o.synth_mixture_rows(77, 5, 16, d, 40, 0.1, stream=1)
    t = pa.Table(ctx, n, d)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    feats = pa.Features(ctx, n)
    u = np.random.default_rng(77).integers(0, 100, n).astype(np.int32)
    feats.set_column("u", pa.F_I32, u)
    feats.set_column("f", pa.F_F32, np.zeros(n, np.float32))
    try:
        def run(qq, k=300, l2=False, counted=None):
            b = ix.stats()
            got = ix.recall_topk_where(feats, "u", "<", 30, qq, k, l2=l2)
            assert_equal_out(got, t.recall_topk_where(feats, "u", "<", 30, qq, k, l2=l2))
            dd = delta(ix, b)
            assert dd["calls"] == 1 and dd["queries"] == qq.shape[0], dd
            for f in FALLBACKS:
                assert dd[f] == (1 if f == counted else 0), (counted, dd)
            return got

        with lifted(ctx):
            assert_equal_out(run(q), oracle_where(tab, q, 300, u < 30))
            # dense: every batch above the limit
            with options(ctx, index_dense_fraction=(0.0, 1e6)):
                run(q, counted="fallback_dense")
                run(q[:1], l2=True, counted="fallback_dense")
            # a non-finite query
            qn = q.copy()
            qn[3, 7] = np.nan
            run(qn, counted="fallback_nonfinite")
            # stale: the table uploaded after the build — the filtered pass answers the new rows
            tab2 = tab.copy()
            tab2[:1000] = o.synth_mixture_rows(78, 0, 1000, d, 40, 0.1)
            t.upload(tab2)
            assert_equal_out(run(q, counted="fallback_stale"), oracle_where(tab2, q, 300, u < 30))
            run(q, l2=True, counted="fallback_stale")
        # a table with a non-finite value: the index builds, every filtered recall takes the filtered pass
        bad = tab[:50_000].copy()
        bad[123, 5] = np.inf
        t2 = pa.Table(ctx, bad.shape[0], d)
        t2.upload(bad)
        ix2 = pa.Index(ctx, t2)
        b = ix2.stats()
        with lifted(ctx):
            got = ix2.recall_topk_where(feats, "u", "<", 30, q, 100)
        assert_equal_out(got, t2.recall_topk_where(feats, "u", "<", 30, q, 100))
        dd = delta(ix2, b)
        assert dd["calls"] == 1 and dd["fallback_nonfinite"] == 1, dd
        ix2.destroy()
        t2.destroy()
        # refusals: the same codes as pg_recall_topk_where
        small = pa.Features(ctx, n // 2)
        small.set_column("u", pa.F_I32, u[:n // 2])
        qb = np.ascontiguousarray(np.tile(q, (17, 1))[:257])
        rows = np.empty(257 * 20000, np.uint64)
        sc = np.empty(257 * 20000, np.float32)
        cnt = np.zeros(257, np.uint32)
        col_u, col_f = feats.index("u"), feats.index("f")
        L = ctx.L

        def codes(fs=feats, col=col_u, op=2, metric=0, queries=qb.ctypes.data, nq=8, k=100, index=ix.h):
            a = L.pg_recall_topk_where(ctx.h, t.h, fs.h, col, op, 30, metric, queries, nq, k, rows.ctypes.data, sc.ctypes.data,
                                       cnt.ctypes.data)
            b = L.pg_index_recall_topk_where(ctx.h, index, fs.h, col, op, 30, metric, queries, nq, k, rows.ctypes.data,
                                             sc.ctypes.data, cnt.ctypes.data)
            return a, b

        assert codes() == (0, 0)
        for kw, want in ((dict(col=-1), -1), (dict(col=99), -1), (dict(op=6), -1), (dict(op=-1), -1), (dict(metric=2), -1),
                         (dict(nq=0), -1), (dict(nq=257), -1), (dict(k=0), -4), (dict(k=16385), -4), (dict(col=col_f), -4),
                         (dict(queries=None), -1), (dict(fs=small, col=small.index("u")), -1)):
            assert codes(**kw) == (want, want), kw
        assert codes(index=None)[1] == -1
        small.destroy()
    finally:
        feats.destroy()
        ix.destroy()
        t.destroy()


def _where_on(c, ix, feats, col, op, value, q, k):
    nq = q.shape[0]
    rows = np.empty((nq, k), np.uint64)
    sc = np.empty((nq, k), np.float32)
    cnt = np.zeros(nq, np.uint32)
    q = np.ascontiguousarray(q, np.float32)
    pa._lib.check(c.L.pg_index_recall_topk_where(c.h, ix.h, feats.h, feats.index(col), OPS[op], int(value), 0, q.ctypes.data, nq, k,
                                                 rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
    return rows, sc, cnt


def test_two_contexts_evicting(ctx, w128):
    """two contexts search one index at once with different filters and a cache of one entry: every call evicts the other
    context's lists while they may be in use, and every answer stays exact"""
    w = w128
    k = 500
    filters = {"a": [("u", "<", 100), ("cl10", "==", 3)], "b": [("u", ">=", 900), ("anti", "==", 0)]}
    qs = {"a": w.q[:16], "b": w.q[16:32]}
    ref = {(n, i): w.t.recall_topk_where(w.feats, *f, qs[n], k) for n, fl in filters.items() for i, f in enumerate(fl)}
    ctx2 = pa.Context(0)
    errs = []
    b = w.ix.where_stats()

    def worker(c, name):
        try:
            for it in range(6):
                i = it % 2
                assert_equal_out(_where_on(c, w.ix, w.feats, *filters[name][i], qs[name], k), ref[(name, i)])
        except BaseException as e:                # noqa: BLE001
            errs.append(e)

    try:
        for c in (ctx, ctx2):
            c.set_option("index_where_cache", 1)
            c.set_option("index_dense_fraction", 1e6)
        th = [threading.Thread(target=worker, args=(ctx, "a")), threading.Thread(target=worker, args=(ctx2, "b"))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        d = where_delta(w.ix, b)
        assert d["evictions"] >= 6 and d["builds"] >= 6, d
    finally:
        ctx.set_option("index_where_cache", CACHE_DEFAULT)
        ctx.set_option("index_dense_fraction", DENSE_DEFAULT)
        ctx2.close()


def test_route_where_through_attached_index(ctx, w64):
    w = w64
    q, k = w.q[:8], 300
    ref = w.t.recall_topk_where(w.feats, "u", "<", 100, q, k)
    ref_l2 = w.t.recall_topk_where(w.feats, "cl10", "==", 3, q, k, l2=True)
    w.ix.attach()
    try:
        with lifted(ctx):
            b = w.ix.stats()
            assert_equal_out(w.t.recall_topk_where(w.feats, "u", "<", 100, q, k), ref)
            assert delta(w.ix, b)["calls"] == 0                       # the default: not routed
            with options(ctx, index_route_where=(1, 0)):
                b = w.ix.stats()
                assert_equal_out(w.t.recall_topk_where(w.feats, "u", "<", 100, q, k), ref)
                assert_equal_out(w.t.recall_topk_where(w.feats, "cl10", "==", 3, q, k, l2=True), ref_l2)
                d = delta(w.ix, b)
                assert d["calls"] == 2 and d["queries"] == 16 and d["pairs_scored"] > 0, d
                assert all(d[f] == 0 for f in FALLBACKS), d
    finally:
        w.ix.detach()
