"""GPU tests of the exact IVF index (pg_index_*): every recall through an index equals the CPU oracle (ids,
order, score bits, counts), pruning is real on clustered tables, and the fallbacks (stale, non-finite, dense) stay exact."""
import threading

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

N, D, CENTRES = 2_000_000, 128, 200
DENSE_DEFAULT = 0.01          # pg_set_option "index_dense_fraction" default
SEED = 0x1D0001


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same(got, orow, osc, l2=False):
    rows, sc, cnt = got
    n = orow.shape[1]
    assert np.array_equal(rows[:, :n], orow)
    assert np.array_equal(bits(sc[:, :n]), bits(osc))
    assert cnt.tolist() == [n] * rows.shape[0]
    if rows.shape[1] > n:
        assert np.all(rows[:, n:] == np.uint64(0xFFFFFFFFFFFFFFFF))
        assert np.all(sc[:, n:] == (np.inf if l2 else -np.inf))


def delta(ix, before):
    after = ix.stats()
    return {k: after[k] - before[k] for k in ("calls", "queries", "pairs_scored", "rows_scored", "fallback_dense", "fallback_stale",
                                              "fallback_nonfinite", "fallback_overflow")}


FALLBACKS = ("fallback_dense", "fallback_stale", "fallback_nonfinite", "fallback_overflow")


class lifted:
    """the dense rule lifted for a block: it is a cost decision calibrated at 100 M rows that sends most batches
    on these small tables to the table's pass, so that without this the search itself would not see the data"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_option("index_dense_fraction", 1e6)

    def __exit__(self, *a):
        self.ctx.set_option("index_dense_fraction", DENSE_DEFAULT)


def assert_served(d, calls=1):
    """every batch of the call was answered by the index search: no fallback of any kind, and pairs were scored"""
    assert d["calls"] == calls and d["pairs_scored"] > 0 and all(d[f] == 0 for f in FALLBACKS), d


def both_rules(ctx, ix, call, ref, l2=False, seen=None):
    """the call under the default dense rule, then again with the rule lifted: exact both times, and the second time served by
    the search.  seen (a list) collects whether the default-rule call reached the search."""
    b = ix.stats()
    assert_same(call(), *ref, l2=l2)
    d = delta(ix, b)
    if seen is not None:
        seen.append(all(d[f] == 0 for f in FALLBACKS))
    b = ix.stats()
    with lifted(ctx):
        assert_same(call(), *ref, l2=l2)
    assert_served(delta(ix, b))


@pytest.fixture(scope="module", params=[0.03, 0.1, 0.3])
def mixture(request, ctx):
    sigma = request.param
    t = pa.Table(ctx, N, D)
    t.fill_mixture(SEED, CENTRES, sigma)
    tab = o.synth_mixture_rows(SEED, 0, N, D, CENTRES, sigma)
    q = o.synth_mixture_rows(SEED, 777, 256, D, CENTRES, sigma, stream=1)
    ip = o.recall_topk(tab, q, 5000)
    l2 = o.recall_topk_l2(tab, q, 5000)
    ix = pa.Index(ctx, t)
    yield sigma, t, tab, q, ip, l2, ix
    ix.destroy()
    t.destroy()


def test_mixture_exact_and_pruned(ctx, mixture):
    sigma, t, tab, q, (orow, osc), (lrow, lsc), ix = mixture
    st = ix.stats()
    assert st["n_lists"] == round(4 * np.sqrt(N)) and st["rows"] == N and st["max_radius"] >= st["mean_radius"] > 0
    for nq in (1, 8, 33, 64, 256):
        for k in (1, 100, 1000, 5000):
            both_rules(ctx, ix, lambda: ix.recall_topk(q[:nq], k), (orow[:nq, :k], osc[:nq, :k]))
    for nq, k in ((1, 5000), (33, 100), (256, 1000)):
        both_rules(ctx, ix, lambda: ix.recall_topk_l2(q[:nq], k), (lrow[:nq, :k], lsc[:nq, :k]), l2=True)
    # the _dev variants
    nq, k = 33, 1000
    dq = ctx.to_device(q[:nq])
    dr, ds = ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 4)
    for l2, (er, es) in ((False, (orow, osc)), (True, (lrow, lsc))):
        cnt = ix.recall_topk_dev(dq, nq, k, dr, ds, l2=l2)
        rows = np.empty((nq, k), np.uint64)
        sc = np.empty((nq, k), np.float32)
        ctx.d2h(rows, dr)
        ctx.d2h(sc, ds)
        assert_same((rows, sc, cnt), er[:nq, :k], es[:nq, :k], l2=l2)
    for p in (dq, dr, ds):
        ctx.free(p)
    if sigma <= 0.1:
        # the pruning itself: the dense rule is a cost decision calibrated at 100 M rows, lifted here so that
        # the pairs of a scan are observed on this 2 M-row table.  One query: a few lists, not the table
        ctx.set_option("index_dense_fraction", 1e6)
        try:
            b = ix.stats()
            assert_same(ix.recall_topk(q[:1], 5000), orow[:1], osc[:1])
            d1 = delta(ix, b)
            # 64 queries
            b = ix.stats()
            assert_same(ix.recall_topk(q[:64], 5000), orow[:64], osc[:64])
            d64 = delta(ix, b)
        finally:
            ctx.set_option("index_dense_fraction", DENSE_DEFAULT)
        assert d1["fallback_dense"] == 0 and d1["fallback_overflow"] == 0
        assert 5000 <= d1["pairs_scored"] <= 0.06 * N, d1
        assert d64["fallback_dense"] == 0 and d64["fallback_overflow"] == 0
        assert d64["pairs_scored"] <= 0.06 * N * 64, d64
    # an explicit list count
    ix2 = pa.Index(ctx, t, n_lists=1024, seed=3)
    assert ix2.stats()["n_lists"] == 1024
    assert_same(ix2.recall_topk(q[:64], 1000), orow[:64, :1000], osc[:64, :1000])
    assert_same(ix2.recall_topk_l2(q[:8], 100), lrow[:8, :100], lsc[:8, :100], l2=True)
    ix2.destroy()


def test_scan_in_several_rounds(ctx):
    """A query whose live lists hold more rows than one round of suspects (2^19 per query): the scan runs in rounds with a select
    between them, the running threshold rises, and the lists chosen for the scan must stay the ones counted after the probe.
    The synchronous call's rounds are not bounded by index_plan_rounds (an attached plan's budget): at 1 it still serves."""
    n, d = 3_000_000, 64
    t = pa.Table(ctx, n, d)
    t.fill_synthetic(o.SEED_TABLE)
    tab = o.synth_rows(o.SEED_TABLE, 0, n, d)
    q = o.synth_rows(o.SEED_QUERY, 0, 4, d)
    ix = pa.Index(ctx, t, n_lists=12)
    ctx.set_option("index_dense_fraction", 1e6)          # wide lists: every batch would otherwise take the table's pass
    try:
        for plan_rounds in (1, 2):                       # (2: the default)
            ctx.set_option("index_plan_rounds", plan_rounds)
            for nq, k in ((1, 5000), (4, 3000)):
                b = ix.stats()
                assert_same(ix.recall_topk(q[:nq], k), *o.recall_topk(tab, q[:nq], k))
                assert_served(delta(ix, b))
            b = ix.stats()
            assert_same(ix.recall_topk_l2(q, 2000), *o.recall_topk_l2(tab, q, 2000), l2=True)
            assert_served(delta(ix, b))
            st = ix.stats()
            assert st["max_query_scan_rows"] > 2 ** 19, st
            assert st["rows_live"] > 0
    finally:
        ctx.set_option("index_dense_fraction", DENSE_DEFAULT)
        ctx.set_option("index_plan_rounds", 2)
    ix.destroy()
    t.destroy()


def test_uniform_table_exact(ctx):
    n, d = 300_000, 128
    t = pa.Table(ctx, n, d)
    t.fill_synthetic(o.SEED_TABLE)
    tab = o.synth_rows(o.SEED_TABLE, 0, n, d)
    q = o.synth_rows(o.SEED_QUERY, 0, 64, d)
    ix = pa.Index(ctx, t)
    for nq, k in ((1, 1000), (64, 100)):
        both_rules(ctx, ix, lambda: ix.recall_topk(q[:nq], k), o.recall_topk(tab, q[:nq], k))
    both_rules(ctx, ix, lambda: ix.recall_topk_l2(q[:8], 500), o.recall_topk_l2(tab, q[:8], 500), l2=True)
    ix.destroy()
    t.destroy()


def _table(ctx, tab, row_offset=0):
    t = pa.Table(ctx, tab.shape[0], tab.shape[1], row_offset)
    t.upload(tab)
    return t


def test_hostile_data(ctx):
    """Every case under the default dense rule (which sends most of them to the table's pass) and again with the rule lifted,
    where the search itself must serve it; the two cases that fall back on purpose assert their own outcome."""
    rng = np.random.default_rng(11)
    d = 128
    seen = []
    # all-equal rows (radius 0, every score tied), rows not a multiple of 64, K > rows
    same = np.tile(rng.standard_normal(d).astype(np.float32), (5003, 1))
    t = _table(ctx, same)
    ix = pa.Index(ctx, t)
    q = rng.standard_normal((4, d)).astype(np.float32)
    for k in (1, 100, 8000):
        both_rules(ctx, ix, lambda: ix.recall_topk(q, k), o.recall_topk(same, q, k), seen=seen)
        both_rules(ctx, ix, lambda: ix.recall_topk_l2(q, k), o.recall_topk_l2(same, q, k), l2=True, seen=seen)
    ix.destroy()
    t.destroy()
    # duplicates and scores tied at the threshold: small-integer rows, many exact ties; zero / one-hot / negated-centroid /
    # huge queries; n_lists 1 and the maximum; a row offset
    base = rng.integers(-2, 3, size=(3000, d)).astype(np.float32)
    tab = np.concatenate([base, base[::-1], base[:77]]).astype(np.float32)
    off = 1_000_003
    t = _table(ctx, tab, off)
    onehot = np.zeros((1, d), np.float32)
    onehot[0, 5] = 1
    qs = np.concatenate([np.zeros((1, d), np.float32), onehot, -tab.mean(0, keepdims=True).astype(np.float32),
                         np.float32(1e30) * np.sign(rng.standard_normal((1, d))).astype(np.float32),
                         rng.integers(-1, 2, size=(4, d)).astype(np.float32)]).astype(np.float32)
    for nl in (1, tab.shape[0] // 64, 17):
        ix = pa.Index(ctx, t, n_lists=nl)
        assert ix.stats()["n_lists"] == nl
        for k in (1, 50, 2000):
            both_rules(ctx, ix, lambda: ix.recall_topk(qs, k), o.recall_topk(tab, qs, k, row_offset=off), seen=seen)
        both_rules(ctx, ix, lambda: ix.recall_topk_l2(qs[:3], 300), o.recall_topk_l2(tab, qs[:3], 300, row_offset=off), l2=True,
                   seen=seen)
        ix.destroy()
    t.destroy()
    # dim 64, 192 and 256 (<= 32 queries per call above 128)
    for dd, nq in ((64, 40), (192, 32), (256, 32)):
        tab = o.synth_mixture_rows(5, 0, 20_011, dd, 20, 0.1)
        q = o.synth_mixture_rows(5, 1, nq, dd, 20, 0.1, stream=1)
        t = _table(ctx, tab)
        ix = pa.Index(ctx, t)
        both_rules(ctx, ix, lambda: ix.recall_topk(q, 700), o.recall_topk(tab, q, 700), seen=seen)
        if dd == 64:
            both_rules(ctx, ix, lambda: ix.recall_topk_l2(q, 700), o.recall_topk_l2(tab, q, 700), l2=True, seen=seen)
        else:
            # squared Euclidean above dim 128 is always `dense` (index.hip: the search has no kernel for it): the table's pass
            # refuses it as it refuses the table's own call, and nothing is counted
            b = ix.stats()
            with lifted(ctx):
                for fn in (lambda: ix.recall_topk_l2(q, 700), lambda: t.recall_topk_l2(q, 700)):
                    with pytest.raises(pa._lib.PgError) as e:
                        fn()
                    assert e.value.code == -4
            assert all(v == 0 for v in delta(ix, b).values())
        ix.destroy()
        t.destroy()
    # a NaN / inf row: builds, every recall is the table's pass (counted), with or without the dense rule
    tab = o.synth_rows(o.SEED_TABLE, 0, 10_000, d)
    tab[17, 3] = np.nan
    tab[9000, 0] = np.inf
    t = _table(ctx, tab)
    ix = pa.Index(ctx, t)
    q = o.synth_rows(o.SEED_QUERY, 0, 3, d)
    b = ix.stats()
    assert_same(ix.recall_topk(q, 100), *t.recall_topk(q, 100)[:2])
    assert delta(ix, b)["fallback_nonfinite"] == 1
    b = ix.stats()
    with lifted(ctx):
        assert_same(ix.recall_topk(q, 100), *t.recall_topk(q, 100)[:2])
    dd = delta(ix, b)
    assert dd["calls"] == 1 and dd["fallback_nonfinite"] == 1 and dd["pairs_scored"] == 0, dd
    ix.destroy()
    t.destroy()
    print("test_hostile_data: %d of %d cases reached the search under the default dense rule, %d of %d with it lifted"
          % (sum(seen), len(seen), len(seen), len(seen)))


def test_outlier_rows_only_the_radius_keeps_live(ctx):
    """Tight clusters; into a few far clusters one row at c + rho q_hat for a query q, so that the row is q's top-1 while its
    list's centroid ranks far down for q.  Only r_L (the outlier widens it) keeps that list live: a bound that under-counts the
    radius prunes the list and loses the top-1.  Exact for IP and L2 with the dense rule lifted, no fallback, and at K = 1 the
    pairs scored show that most of the table was pruned."""
    rng = np.random.default_rng(0x0071)
    d, n_c, per, nq = 128, 64, 4096, 8
    cent = rng.standard_normal((n_c, d))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    tab = (np.repeat(cent, per, axis=0) + 0.02 * rng.standard_normal((n_c * per, d)) / np.sqrt(d)).astype(np.float32)
    q = rng.standard_normal((nq, d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cq = q @ cent.T                                          # [nq][n_c]
    far = []
    for j in range(nq):                                      # a distinct far cluster per query: among the lowest c.q
        far.append(next(c for c in np.argsort(cq[j]) if c not in far))
    rho = cq.max(axis=1) - cq[np.arange(nq), far] + 0.3
    out_rows = np.array([f * per + 17 for f in far])
    tab[out_rows] = (cent[far] + rho[:, None] * q).astype(np.float32)
    q = q.astype(np.float32)
    t = _table(ctx, tab)
    ix = pa.Index(ctx, t, n_lists=4 * n_c, iters=16)          # (several lists per cluster: few lists span two clusters)
    try:
        st = ix.read()
        list_of = np.empty(tab.shape[0], np.int64)
        list_of[st["perm"].astype(np.int64)] = np.repeat(np.arange(4 * n_c), np.diff(st["offsets"].astype(np.int64)))
        crank = np.argsort(np.argsort(-(q.astype(np.float64) @ st["centroids"].T.astype(np.float64)), axis=1), axis=1)
        for j in range(nq):
            assert crank[j, list_of[out_rows[j]]] >= 2 * n_c, "the outlier's list must rank far down for its query"
        ip = o.recall_topk(tab, q, 5000)
        assert np.array_equal(ip[0][:, 0], out_rows.astype(np.uint64)), "the outlier must be its query's top-1"
        l2 = o.recall_topk_l2(tab, q, 5000)
        with lifted(ctx):
            # (pruning is measured at K = 1: at larger K the wide outlier lists, whose bounds are the highest, fill the probe
            # and set a low threshold — exact, but most of the table is scanned)
            for k in (1, 100, 5000):
                b = ix.stats()
                assert_same(ix.recall_topk(q, k), ip[0][:, :k], ip[1][:, :k])
                dd = delta(ix, b)
                assert_served(dd)
                assert k > 1 or dd["pairs_scored"] <= 0.2 * tab.shape[0] * nq, dd
                b = ix.stats()
                assert_same(ix.recall_topk_l2(q, k), l2[0][:, :k], l2[1][:, :k], l2=True)
                dd = delta(ix, b)
                assert_served(dd)
                assert k > 1 or dd["pairs_scored"] <= 0.2 * tab.shape[0] * nq, dd
    finally:
        ix.destroy()
        t.destroy()


def test_k_above_rows_with_a_row_offset(ctx):
    """K above the table's row count through the search (the dense rule lifted): every row, padded with UINT64_MAX and -inf
    (+inf for L2), counts = rows, global ids offset"""
    n, d, off = 5_003, 64, 4_000_000_007              # (global ids are 32-bit)
    tab = o.synth_mixture_rows(13, 0, n, d, 16, 0.05)
    q = o.synth_mixture_rows(13, 2, 6, d, 16, 0.05, stream=1)
    t = _table(ctx, tab, off)
    for nl in (1, 9, n // 64):
        ix = pa.Index(ctx, t, n_lists=nl)
        try:
            with lifted(ctx):
                for k in (n, n + 1, 8000):
                    b = ix.stats()
                    got = ix.recall_topk(q, k)
                    assert_same(got, *o.recall_topk(tab, q, k, row_offset=off))
                    assert got[2].tolist() == [n] * q.shape[0]
                    assert_served(delta(ix, b))
                    b = ix.stats()
                    assert_same(ix.recall_topk_l2(q, k), *o.recall_topk_l2(tab, q, k, row_offset=off), l2=True)
                    assert_served(delta(ix, b))
        finally:
            ix.destroy()
    t.destroy()


def test_generations_refusals_and_no_side_effects(ctx):
    d, n = 128, 100_000
    tab = o.synth_mixture_rows(9, 0, n, d, 50, 0.05)
    q = o.synth_mixture_rows(9, 3, 8, d, 50, 0.05, stream=1)
    t = _table(ctx, tab)
    before = t.recall_topk(q, 500)
    ix = pa.Index(ctx, t)
    assert_same(ix.recall_topk(q, 500), *o.recall_topk(tab, q, 500))
    after = t.recall_topk(q, 500)               # the table's own recall is untouched by the index
    assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1]))
    # a changed table: the stale index serves the new rows through the table's pass
    new = tab.copy()
    new[:5000] = -new[:5000]
    t.upload(new[:5000], 0)
    b = ix.stats()
    assert_same(ix.recall_topk(q, 500), *o.recall_topk(new, q, 500))
    assert delta(ix, b)["fallback_stale"] == 1
    ix.destroy()
    ix = pa.Index(ctx, t)                         # rebuilt: pruning is back (observed with the dense rule lifted)
    ctx.set_option("index_dense_fraction", 1e6)
    try:
        b = ix.stats()
        assert_same(ix.recall_topk(q[:1], 500), *o.recall_topk(new, q[:1], 500))
        dd = delta(ix, b)
    finally:
        ctx.set_option("index_dense_fraction", DENSE_DEFAULT)
    assert dd["fallback_stale"] == 0 and dd["fallback_dense"] == 0 and dd["pairs_scored"] < n // 4
    # refusals
    with pytest.raises(pa._lib.PgError) as e:
        ix.recall_topk(q, 0)
    assert e.value.code == -4
    with pytest.raises(pa._lib.PgError) as e:
        ix.recall_topk(q, 16385)
    assert e.value.code == -4
    rows = np.zeros((257, 10), np.uint64)
    sc = np.zeros((257, 10), np.float32)
    cnt = np.zeros(257, np.uint32)
    qq = np.zeros((257, d), np.float32)
    assert ctx.L.pg_index_recall_topk(ctx.h, ix.h, qq.ctypes.data, 257, 10, rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == -1
    assert ctx.L.pg_index_recall_topk(ctx.h, ix.h, qq.ctypes.data, 0, 10, rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == -1
    assert ctx.L.pg_index_recall_topk(ctx.h, None, qq.ctypes.data, 1, 10, rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == -1
    feats = pa.Features(ctx, n)
    feats.set_column("c", pa.F_I32, np.arange(n, dtype=np.int32) % 3)
    v = t.view(feats, "c", "==", 1)
    with pytest.raises(pa._lib.PgError) as e:
        pa.Index(ctx, v)
    assert e.value.code == -4
    v.destroy()
    feats.destroy()
    ix.destroy()
    t.destroy()


def test_two_contexts_share_one_index(ctx):
    d, n = 128, 400_000
    tab = o.synth_mixture_rows(21, 0, n, d, 100, 0.1)
    q = o.synth_mixture_rows(21, 4, 64, d, 100, 0.1, stream=1)
    t = _table(ctx, tab)
    ix = pa.Index(ctx, t)
    ref = o.recall_topk(tab, q, 1000)
    ctx2 = pa.Context(0)
    out, errs = {}, []

    def worker(c, name, sl):
        try:
            for _ in range(3):
                out[name] = _recall_on(c, ix, q[sl], 1000)
        except Exception as e:                    # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=worker, args=(ctx, "a", slice(0, 32))), threading.Thread(target=worker, args=(ctx2, "b", slice(32, 64)))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    assert_same(out["a"], ref[0][:32], ref[1][:32])
    assert_same(out["b"], ref[0][32:], ref[1][32:])
    ctx2.close()
    ix.destroy()
    t.destroy()


def _recall_on(c, ix, q, k):
    nq = q.shape[0]
    rows = np.empty((nq, k), np.uint64)
    sc = np.empty((nq, k), np.float32)
    cnt = np.zeros(nq, np.uint32)
    q = np.ascontiguousarray(q, np.float32)
    pa._lib.check(c.L.pg_index_recall_topk(c.h, ix.h, q.ctypes.data, nq, k, rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
    return rows, sc, cnt
