"""GPU tests of pg_index_refresh: after a refresh — incremental from the table's write log, or full on the matrix
pipe — the index's arrays are what the build's steps give for the kept centroids and the current rows (the rule restated in
tests/index_refresh_ref.py through the oracle's chains), and every recall through it equals the oracle on the current rows.
Covered: the write log's limits, a fill and a swap, an attached index refreshed while a coalescer serves, hostile magnitudes and a
NaN row, and a table that makes the screen useless.  Every comparison is against the oracle, never against the code under test."""
import threading

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

from index_bound_ref import _adversarial, _up32
import index_refresh_ref as ref

pytestmark = pytest.mark.gpu

DENSE_DEFAULT = 0.01
PG_ERR_UNSUPPORTED = -4
FALLBACKS = ("fallback_dense", "fallback_stale", "fallback_nonfinite", "fallback_overflow")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def like_oracle(got, orow, osc):
    assert np.array_equal(got[0], orow)
    assert np.array_equal(bits(got[1]), bits(osc))


def oracle_where(tab, q, k, mask, l2=False):
    ids = np.flatnonzero(mask)
    orow, osc = (o.recall_topk_l2 if l2 else o.recall_topk)(tab[ids], q, k)
    return ids[orow.astype(np.int64)].astype(np.uint64), osc


class lifted:
    """the dense rule is a cost decision calibrated at 100 M rows: lifted so that the search itself serves"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_option("index_dense_fraction", 1e6)

    def __exit__(self, *a):
        self.ctx.set_option("index_dense_fraction", DENSE_DEFAULT)


def delta(fn, before):
    after = fn()
    return {k: after[k] - before[k] for k in after}


def check_rule(ix, tab, cent=None, cnorm=None):
    """Index.read() equals the rule on the current rows and the read centroids: offsets and perm exactly, the radius within two
    fp32 steps above the fp64 maximum distance of the list's rows, 0 for an empty list; centroids and cnorm unchanged"""
    r = ix.read()
    if cent is not None:
        assert np.array_equal(bits(r["centroids"]), bits(cent)) and np.array_equal(bits(r["cnorm"]), bits(cnorm))
    lists, offsets, perm, far = ref.rule_index(tab, r["centroids"])
    assert np.array_equal(r["offsets"], offsets)
    assert np.array_equal(r["perm"], perm)
    sizes = np.diff(offsets.astype(np.int64))
    assert np.all(r["radius"][sizes == 0] == 0)
    finite = np.ones(len(sizes), bool)
    finite[lists[~np.all(np.isfinite(tab), axis=1)]] = False      # (a list with a non-finite row has no measured radius)
    full = (sizes > 0) & finite
    rad = r["radius"][full]
    assert np.all(rad.astype(np.float64) >= far[full])
    top = np.nextafter(_up32(far[full] * (1 + 2.0 ** -40)).astype(np.float32), np.float32(np.inf))     # (as tests/test_gpu_index_bounds.py)
    assert np.all(rad <= top)
    st = ix.stats()
    assert st["largest_list"] == sizes.max() and st["empty_lists"] == int(np.sum(sizes == 0))
    if finite.all():
        assert st["max_radius"] == r["radius"].max()
    return r, lists


def check_recalls(ctx, ix, t, tab, q, k, feats=None, mask=None, pruned=True):
    """inner product and squared Euclidean, plain and filtered, equal the oracle on `tab`; no fallback; pruning is real"""
    n = tab.shape[0]
    with lifted(ctx):
        for l2 in (False, True):
            s0 = ix.stats()
            got = ix.recall_topk_l2(q, k) if l2 else ix.recall_topk(q, k)
            like_oracle(got, *(o.recall_topk_l2(tab, q, k) if l2 else o.recall_topk(tab, q, k)))
            d = delta(ix.stats, s0)
            assert all(d[f] == 0 for f in FALLBACKS), d
            if pruned:                                      # (the bar tests/test_gpu_index.py uses on these tables: one query)
                s0 = ix.stats()
                got = ix.recall_topk_l2(q[:1], k) if l2 else ix.recall_topk(q[:1], k)
                like_oracle(got, *(o.recall_topk_l2(tab, q[:1], k) if l2 else o.recall_topk(tab, q[:1], k)))
                assert delta(ix.stats, s0)["pairs_scored"] < n // 4
            if feats is not None:
                s0 = ix.stats()
                got = ix.recall_topk_where(feats, "u", "<", 500, q, k, l2=l2)
                like_oracle(got, *oracle_where(tab, q, k, mask, l2))
                d = delta(ix.stats, s0)
                assert all(d[f] == 0 for f in FALLBACKS), d


@pytest.fixture(scope="module", params=ref.GPU_TABLES, ids=lambda p: "dim%d" % p[2])
def world(ctx, request):
    seed, n, dim, centres, sigma = request.param
    tab = o.synth_mixture_rows(seed, 0, n, dim, centres, sigma)
    q = o.synth_mixture_rows(seed, 2, 16, dim, centres, sigma, stream=1)
    t = pa.Table(ctx, n, dim)
    t.fill_mixture(seed, centres, sigma)
    ix = pa.Index(ctx, t)
    yield request.param, t, tab, q, ix
    ix.destroy()
    t.destroy()


def test_noop_and_forced_full_refresh_reproduces_the_build(ctx, world):
    (seed, n, dim, centres, sigma), t, tab, q, ix = world
    built = ix.read()
    st0, r0 = ix.stats(), ix.refresh_stats()
    ix.refresh()                                           # current: nothing to do
    d = delta(ix.refresh_stats, r0)
    assert d["refreshes"] == 1 and d["noop"] == 1 and d["full"] == 0 and d["incremental"] == 0
    ix.refresh(force=True)
    d = delta(ix.refresh_stats, r0)
    assert d["full"] == 1 and d["rows_reassigned"] == n and d["rows_moved"] == 0, d
    assert d["rows_confirmed_wide"] <= n // 100, d          # (a condition: tests/test_index_refresh_cpu.py evaluates it on the CPU)
    rs = ix.refresh_stats()
    assert rs["last_generation"] == st0["generation"] and rs["last_ms"] > 0 and rs["last_assign_ms"] > 0
    again = ix.read()
    for name in ("offsets", "perm", "centroids", "cnorm", "radius"):
        assert np.array_equal(bits(again[name]), bits(built[name])), name
    st1 = ix.stats()
    for name in ("generation", "build_ms", "max_radius", "mean_radius", "largest_list", "empty_lists"):
        assert st1[name] == st0[name], name
    check_rule(ix, tab, built["centroids"], built["cnorm"])
    check_recalls(ctx, ix, t, tab, q, 500)


def test_incremental_refresh_after_an_upload(ctx, world):
    (seed, n, dim, centres, sigma), t0, tab0, q, ix0 = world
    k = 500
    t = pa.Table(ctx, n, dim)
    t.upload(tab0)
    ix = pa.Index(ctx, t)
    feats = pa.Features(ctx, n)
    u = np.random.default_rng(seed).integers(0, 1000, n).astype(np.int32)
    feats.set_column("u", pa.F_I32, u)
    try:
        built = ix.read()
        tab = tab0.copy()
        tab[1000:1016] = q                                  # the queries' own vectors land in the table: the answers change
        t.upload(tab[1000:1016], row0=1000)
        s0 = ix.stats()
        like_oracle(ix.recall_topk(q, k), *o.recall_topk(tab, q, k))
        assert delta(ix.stats, s0)["fallback_stale"] == 1
        r0 = ix.refresh_stats()
        ix.refresh()
        d = delta(ix.refresh_stats, r0)
        assert d["incremental"] == 1 and d["full"] == 0 and d["rows_reassigned"] == 16 and d["rows_moved"] <= 16, d
        assert ix.stats()["generation"] == ix.refresh_stats()["last_generation"] != s0["generation"]
        check_recalls(ctx, ix, t, tab, q, k, feats, u < 500)
        inc, _ = check_rule(ix, tab, built["centroids"], built["cnorm"])
        # the two modes are interchangeable
        r1 = ix.refresh_stats()
        ix.refresh(mode="full", force=True)
        d = delta(ix.refresh_stats, r1)
        assert d["full"] == 1 and d["rows_moved"] == 0 and d["rows_confirmed_wide"] <= n // 100, d
        full, _ = check_rule(ix, tab, built["centroids"], built["cnorm"])
        for name in ("offsets", "perm", "radius"):
            assert np.array_equal(bits(full[name]), bits(inc[name])), name
        check_recalls(ctx, ix, t, tab, q, k, feats, u < 500)
    finally:
        feats.destroy()
        ix.destroy()
        t.destroy()


def test_full_refresh_after_a_fill_and_a_swap(ctx, world):
    (seed, n, dim, centres, sigma), t0, tab0, q, ix0 = world
    k = 300
    t = pa.Table(ctx, n, dim)
    t.fill_mixture(seed, centres, sigma)
    ix = pa.Index(ctx, t)
    t2 = pa.Table(ctx, n, dim)
    try:
        built = ix.read()
        # every row new, same distribution
        t.fill_mixture(seed + 7, centres, sigma)
        tab = o.synth_mixture_rows(seed + 7, 0, n, dim, centres, sigma)
        r0 = ix.refresh_stats()
        ix.refresh()
        d = delta(ix.refresh_stats, r0)
        assert d["full"] == 1 and d["incremental"] == 0 and d["rows_reassigned"] == n and d["rows_moved"] > 0, d
        assert d["rows_confirmed_wide"] <= n // 100, d
        check_rule(ix, tab, built["centroids"], built["cnorm"])
        check_recalls(ctx, ix, t, tab, q, k, pruned=False)
        # a second table swapped in
        t2.fill_mixture(seed + 9, centres, sigma)
        tab2 = o.synth_mixture_rows(seed + 9, 0, n, dim, centres, sigma)
        t.swap(t2)
        s0 = ix.stats()
        like_oracle(ix.recall_topk(q, k), *o.recall_topk(tab2, q, k))
        assert delta(ix.stats, s0)["fallback_stale"] == 1
        r0 = ix.refresh_stats()
        ix.refresh()
        d = delta(ix.refresh_stats, r0)
        assert d["full"] == 1 and d["incremental"] == 0, d
        check_rule(ix, tab2, built["centroids"], built["cnorm"])
        check_recalls(ctx, ix, t, tab2, q, k, pruned=False)
    finally:
        ix.destroy()
        t2.destroy()
        t.destroy()


def test_log_limits(ctx):
    seed, n, dim, centres, sigma = ref.GPU_TABLES[0]
    tab = o.synth_mixture_rows(seed, 0, n, dim, centres, sigma)
    q = o.synth_mixture_rows(seed, 2, 16, dim, centres, sigma, stream=1)
    t = pa.Table(ctx, n, dim)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    try:
        built = ix.read()
        # adjacent and overlapping uploads merge into one range: an incremental refresh of their union
        for row0 in (5000, 5008, 5004):
            tab[row0:row0 + 8] = tab[row0 + 100_000:row0 + 100_008]
            t.upload(tab[row0:row0 + 8], row0=row0)
        r0 = ix.refresh_stats()
        ix.refresh(mode="incremental")
        d = delta(ix.refresh_stats, r0)
        assert d["incremental"] == 1 and d["rows_reassigned"] == 16, d
        check_rule(ix, tab, built["centroids"], built["cnorm"])
        # 70 disjoint small uploads overflow the log's 64 ranges
        for i in range(70):
            row0 = 1000 + 2000 * i
            tab[row0:row0 + 4] = tab[row0 + 50:row0 + 54]
            t.upload(tab[row0:row0 + 4], row0=row0)
        r0, gen = ix.refresh_stats(), ix.stats()["generation"]
        with pytest.raises(pa._lib.PgError) as err:
            ix.refresh(mode="incremental")
        assert err.value.code == PG_ERR_UNSUPPORTED
        d = delta(ix.refresh_stats, r0)
        assert d["refreshes"] == 0 and ix.stats()["generation"] == gen
        s0 = ix.stats()                                     # still stale, still usable
        like_oracle(ix.recall_topk(q, 100), *o.recall_topk(tab, q, 100))
        assert delta(ix.stats, s0)["fallback_stale"] == 1
        ix.refresh()
        d = delta(ix.refresh_stats, r0)
        assert d["full"] == 1 and d["incremental"] == 0 and d["rows_reassigned"] == n, d
        check_rule(ix, tab, built["centroids"], built["cnorm"])
        check_recalls(ctx, ix, t, tab, q, 100)
        # past "index_refresh_full_fraction" of the rows auto mode refreshes in full (and the table drops its log)
        ctx.set_option("index_refresh_full_fraction", 0.001)
        try:
            tab[20_000:20_400] = tab[120_000:120_400]
            t.upload(tab[20_000:20_400], row0=20_000)
            r0 = ix.refresh_stats()
            ix.refresh()
            assert delta(ix.refresh_stats, r0)["full"] == 1
        finally:
            ctx.set_option("index_refresh_full_fraction", 0.1)
        check_rule(ix, tab, built["centroids"], built["cnorm"])
    finally:
        ix.destroy()
        t.destroy()


def test_attached_index_refreshed_while_a_coalescer_serves(ctx):
    seed, n, dim, centres, sigma = ref.GPU_TABLES[0]
    k = 200
    tab = o.synth_mixture_rows(seed, 0, n, dim, centres, sigma)
    q = o.synth_mixture_rows(seed, 2, 16, dim, centres, sigma, stream=1)
    tab2 = tab.copy()
    tab2[1000:1016] = q
    old, new = o.recall_topk(tab, q, k), o.recall_topk(tab2, q, k)
    t = pa.Table(ctx, n, dim)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    ctx.set_option("index_dense_fraction", 1e6)
    ix.attach()
    co = pa.Coalescer(ctx, t, k, max_wait_us=500)
    try:
        s0 = ix.serving_stats()
        like_oracle(t.recall_topk(q, k), *old)
        assert delta(ix.serving_stats, s0)["plans_held"] == 1
        answers, errs, stop = [], [], threading.Event()

        def caller(i):
            try:
                while not stop.is_set():
                    answers.append((i, co.recall(q[i])))
            except BaseException as e:          # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=caller, args=(i,)) for i in range(8)]
        for x in th:
            x.start()
        try:
            t.upload(tab2[1000:1016], row0=1000)
            s1 = ix.serving_stats()
            like_oracle(t.recall_topk(q, k), *new)
            assert delta(ix.serving_stats, s1)["skipped_stale"] >= 1
            ix.refresh()
            s2 = ix.serving_stats()
            like_oracle(t.recall_topk(q, k), *new)
            d = delta(ix.serving_stats, s2)
            assert d["plans_held"] >= 1 and d["skipped_stale"] == 0, d
        finally:
            stop.set()
            for x in th:
                x.join(60)
        assert not any(x.is_alive() for x in th), "a coalescer caller did not return"
        assert not errs, errs
        assert len(answers) >= 8
        for i, (rows, sc, cnt) in answers:                  # the rows of ONE generation, old or new: never a mixture
            assert cnt == k
            hit = [np.array_equal(rows, w[0][i]) and np.array_equal(bits(sc), bits(w[1][i])) for w in (old, new)]
            assert any(hit), i
        assert ix.refresh_stats()["incremental"] == 1
    finally:
        co.destroy()
        ix.detach()
        ctx.set_option("index_dense_fraction", DENSE_DEFAULT)
        ix.destroy()
        t.destroy()


def clustered(rng, n, dim, scale):
    """rows around 40 centres, every value multiplied by `scale` (fp32)"""
    c = rng.standard_normal((40, dim))
    x = c[rng.integers(0, 40, n)] + 0.1 * rng.standard_normal((n, dim))
    with np.errstate(all="ignore"):
        return (x * scale).astype(np.float32)


@pytest.mark.parametrize("scale", (1e-18, 1e17, 3e-39 * 2.0 ** 20), ids=("1e-18", "1e17", "denormal"))
def test_hostile_scales(ctx, scale):
    n, dim, k = 20_000, 64, 50
    rng = np.random.default_rng(0x1F05)
    tab = clustered(rng, n, dim, scale)
    q = tab[rng.integers(0, n, 8)].copy()
    t = pa.Table(ctx, n, dim)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    try:
        built = ix.read()
        gen = ix.stats()["generation"]
        s0 = ix.stats()
        ix.recall_topk(q, k)
        fb_built = {f: delta(ix.stats, s0)[f] for f in FALLBACKS}
        tab[300:364] = tab[9000:9064]
        t.upload(tab[300:364], row0=300)
        for mode, force in (("incremental", False), ("full", True)):
            ix.refresh(mode=mode, force=force)
            check_rule(ix, tab, built["centroids"], built["cnorm"])
            s0 = ix.stats()
            got = ix.recall_topk(q, k)
            want = t.recall_topk(q, k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
            like_oracle(got, *o.recall_topk(tab, q, k))
            d = delta(ix.stats, s0)
            assert d["fallback_stale"] == 0
            assert {f: d[f] for f in FALLBACKS} == fb_built      # the fallbacks counted as after a build
        assert ix.stats()["generation"] != gen
    finally:
        ix.destroy()
        t.destroy()


def test_nan_row(ctx):
    n, dim, k = 20_000, 128, 50
    rng = np.random.default_rng(0x1F06)
    tab = clustered(rng, n, dim, 1.0)
    q = tab[rng.integers(0, n, 8)].copy()
    t = pa.Table(ctx, n, dim)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    try:
        built = ix.read()
        tab[123, 7] = np.nan
        tab[124, :] = np.inf
        t.upload(tab[123:125], row0=123)
        for mode, force in (("incremental", False), ("full", True)):
            ix.refresh(mode=mode, force=force)
            r, lists = check_rule(ix, tab, built["centroids"], built["cnorm"])
            assert lists[123] == 0 and 123 in r["perm"][r["offsets"][0]:r["offsets"][1]]
            s0 = ix.stats()
            got, want = ix.recall_topk(q, k), t.recall_topk(q, k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
            d = delta(ix.stats, s0)
            assert d["fallback_nonfinite"] == 1 and d["fallback_stale"] == 0, d
        # finite again: the incremental path notices (it looks at every row once the index was non-finite)
        tab[123:125] = tab[200:202]
        t.upload(tab[123:125], row0=123)
        ix.refresh(mode="incremental")
        check_rule(ix, tab, built["centroids"], built["cnorm"])
        with lifted(ctx):
            s0 = ix.stats()
            like_oracle(ix.recall_topk(q, k), *o.recall_topk(tab, q, k))
            d = delta(ix.stats, s0)
            assert all(d[f] == 0 for f in FALLBACKS), d
    finally:
        ix.destroy()
        t.destroy()


@pytest.mark.parametrize("dim", (64, 128))
def test_screen_on_the_device_stays_inside_its_bound(ctx, dim):
    """What the equality of the two modes rests on: the matrix pipe's screen value lies within e(x, L) of the
    rule's distance.  pg_index_screen_probe runs the assignment's own loads, MFMA sequence and formulas; the rule's distance is the
    oracle's chain.  Operands whose products all have one sign (every addition rounds a growing sum: the accumulation's worst
    case), at magnitudes across the range, and the adversarial lists of tests/index_bound_ref.py.  The device's e equals the
    numpy restatement (the constants and the range test of index_assign.hip against tests/index_refresh_ref.py)."""
    rng = np.random.default_rng(0x1F08 + dim)
    worst = 0.0
    for scale in (1e-4, 0.03, 1.0, 37.0, 1e3, 3e5):
        # sign-aligned: |values| in [0.5, 1) x scale (every bf16 lo part in use), one sign pattern for rows and centroids
        sign = np.sign(rng.standard_normal(dim)).astype(np.float32)
        rows = (rng.uniform(0.5, 1.0, (96, dim)) * scale).astype(np.float32) * sign
        cent = (rng.uniform(0.5, 1.0, (70, dim)) * scale).astype(np.float32) * sign
        cent[1::2] *= -1                                                   # ... and every product negative for the odd lists
        x, c, q = _adversarial(dim, scale, rng)
        rows = np.concatenate([rows, x, q]).astype(np.float32)
        cent = np.concatenate([cent, c[None, :], x[:25]]).astype(np.float32)
        s, e = pa.index_screen_probe(ctx, rows, cent)
        ok = ref.in_range(rows)
        assert ref.in_range(cent).all()
        assert np.array_equal(np.isfinite(e), np.broadcast_to(ok[:, None], e.shape))          # the same range test
        cn2 = ref.chain_norm2(cent)
        d = ref.rule_dist(rows, cent, cn2)
        e_ref = ref.bound(rows[ok], cent, cn2)
        assert np.allclose(e[ok], e_ref, rtol=1e-6, atol=0)                # (fp32 evaluation order: an ulp or two)
        err = np.abs(s[ok].astype(np.float64) - d[ok].astype(np.float64))
        ratio = float(np.max(err / e[ok]))
        print("dim %d scale %g: max |screen - rule| / e = %.4f" % (dim, scale, ratio))
        assert np.all(err <= e[ok].astype(np.float64)), (scale, ratio)
        worst = max(worst, ratio)
    assert 0.0 < worst <= 1.0


def test_screen_useless(ctx):
    """every row within 2^-20 (relative) of one vector: the centroids are near-duplicates, every list lies within the bound of
    every other, the slots overflow — the rows go through the fp32 kernel and the lists are still the rule's"""
    n, dim = 20_000, 64
    rng = np.random.default_rng(0x1F07)
    v = rng.standard_normal(dim)
    tab = (v[None, :] * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, (n, dim)))).astype(np.float32)
    t = pa.Table(ctx, n, dim)
    t.upload(tab)
    ix = pa.Index(ctx, t)
    try:
        built = ix.read()
        r0 = ix.refresh_stats()
        ix.refresh(force=True)
        d = delta(ix.refresh_stats, r0)
        assert d["full"] == 1 and d["rows_confirmed_wide"] > 0, d
        again, _ = check_rule(ix, tab, built["centroids"], built["cnorm"])
        for name in ("offsets", "perm", "radius"):
            assert np.array_equal(bits(again[name]), bits(built[name])), name
        q = tab[:4].copy()
        got = ix.recall_topk(q, 20)
        like_oracle(got, *o.recall_topk(tab, q, 20))
    finally:
        ix.destroy()
        t.destroy()
