"""GPU tests of the U2I2X2I recall (csrc/x2i.hip) against tests/x2i_ref.py: ids, fp64 score BITS, counts and padding
must be equal.  One X table (tests/x2i_cases.py) over an item table of 70 001 x 64 rows — just past 65 536 — with a nonzero
row_offset and 4 200 X: a random body, crafted regions (an X shared by 256 rows, an item shared by 300 X, keys that collide in the
kernel's three hash tables, lists at every limit) and a band of rows and of X never uploaded."""
import numpy as np
import pytest

import cf_ref
import fanin_ref
import pairec_amd as pa
import rtu2i_cases
import x2i_cases as cases
import x2i_ref as ref
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

ROWS, N_X, ROW_OFFSET, DIM = cases.ROWS, cases.N_X, cases.ROW_OFFSET, 64
U32MAX = cases.U32MAX


def assert_same(got, want):
    assert np.array_equal(np.asarray(got[2], np.uint32), np.asarray(want[2], np.uint32))
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))


class Pair:
    """a device X table and its host restatement, uploaded together"""

    def __init__(self, ctx, table, rows, n_x, row_offset):
        self.dev = pa.XTable(ctx, table, n_x)
        self.host = ref.XLists(rows, n_x, row_offset)

    def upload_item2x(self, off, ids, row0=0):
        self.dev.upload_item2x(off, ids, row0)
        self.host.upload_item2x(off, ids, row0)

    def upload_x2item(self, off, rows, scores, x0=0):
        self.dev.upload_x2item(off, rows, scores, x0)
        self.host.upload_x2item(off, rows, scores, x0)

    def check(self, triggers, prefer, k, normalize=True, max_rule=False, lists=None):
        got = self.dev.x2i_recall(triggers, prefer, k, normalize, max_rule, lists)
        assert_same(got, ref.x2i_recall(self.host, triggers, prefer, k, normalize, max_rule, lists))
        return got


@pytest.fixture(scope="module")
def base(ctx):
    t = pa.Table(ctx, ROWS, DIM, ROW_OFFSET)
    p = Pair(ctx, t, ROWS, N_X, ROW_OFFSET)
    cases.upload(p, cases.build())
    yield p
    p.dev.destroy()
    t.destroy()


def pairs_of(base, trig):
    return sum(len(base.host.x2i.get(x, ((), ()))[0]) for x, _ in ref.hop1(base.host, trig, np.ones(len(trig))))


# ---- the grid: accumulation, ordering, edges (the same requests pg_x2i_recall_host answers in test_x2i_cpu.py) ---------------------------

@pytest.mark.parametrize("name", sorted(cases.grid()))
def test_grid(base, name):
    trig, pref, k, normalize, max_rule = cases.grid()[name]
    got = base.check(trig, pref, k, normalize, max_rule)
    if name.startswith("shared_x_256"):
        assert 50 <= got[2][0] <= 60                               # 256 ordered additions onto X 2000 .. 2004, their items behind them
    if name == "shared_item_fan":
        assert got[2][0] == 5 and not np.array_equal(got[1][0], got[1][1])    # the same terms in the other order: other bits
    if name in ("addition_order_x", "addition_order_item"):
        assert got[1][0][0] != got[1][1][0]
    if name == "wide_and_many":
        assert len(ref.hop1(base.host, trig[0], [1.0])) == 64 and len(ref.hop1(base.host, trig[1], np.ones(16))) == 1024
        assert got[2][1] > 2000
    if name.startswith("ties"):
        sc = got[1][0][:got[2][0]]
        tie = np.nonzero(sc[1:] == sc[:-1])[0]
        assert len(tie) > 0 and np.all(got[0][0][tie] < got[0][0][tie + 1])
    if name == "negative":
        assert np.all(got[1][0][:got[2][0]] < 0)                   # every score negative: m stays 0, nothing is divided
        assert_same(got, base.dev.x2i_recall(trig, pref, k, False))
        assert np.signbit(got[1][1][:got[2][1]]).any() and (got[1][1][:got[2][1]] == 0).any()   # -0.0 keeps its bits
    if name == "edges":
        assert list(got[2][:6]) == [0, 0, 0, 0, 0, 0] and got[2][7] == 0 and got[2][8] == 1 and got[2][9] == 5 and got[2][13] == 1024
        assert got[0][8][0] == ROW_OFFSET + cases.R_SELF + 1


def test_k_edges(base):
    rng = np.random.default_rng(24)
    trig = [cases.R_WIDE, cases.R_DYADIC, cases.R_COLLIDE + 1]
    pref = cases.wide_prefer(rng, len(trig))
    distinct = len(ref.accumulate(base.host, trig, pref))
    assert distinct > 100
    for k in (1, distinct, distinct + 1, 16384):
        got = base.check([trig], [pref], k)
        assert got[2][0] == min(k, distinct)


# ---- batching and tiers --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(base):
    trig, pref = cases.mixed()
    assert pairs_of(base, trig[9]) > cases.KNOB_DEFAULT and pairs_of(base, trig[10]) == cases.LDS_MAX_PAIRS
    return trig, pref, ref.x2i_recall(base.host, trig, pref, 200, True)


def test_mixed_batch_of_256(base, mixed):
    trig, pref, want = mixed
    assert_same(base.dev.x2i_recall(trig, pref, 200), want)
    assert want[2].max() == 200 and (want[2] == 0).sum() >= 32


def test_batching_invariance(base, mixed):
    trig, pref, want = mixed
    for q in (7, 9, 40):
        assert_same(base.dev.x2i_recall([trig[q]], [pref[q]], 200), tuple(w[q:q + 1] for w in want))


def test_both_tiers_give_one_answer(ctx, base, mixed):
    trig, pref, want = mixed
    rng = np.random.default_rng(32)
    # at the LDS tier's limit, one pair past it, and colliding keys in both
    long5 = list(range(cases.R_LONG, cases.R_LONG + 5))
    edge = [long5[:4] + [cases.R_DYADIC], long5, long5 + [cases.R_ONE], [cases.R_COLLIDE + j for j in range(5)], [cases.R_XCOLLIDE]]
    assert [pairs_of(base, t) for t in edge[:3]] == [4096 + 20, cases.LDS_MAX_PAIRS, cases.LDS_MAX_PAIRS + 1]
    epref = [cases.wide_prefer(rng, len(t)) for t in edge]
    ewant = ref.x2i_recall(base.host, edge, epref, 6000, True)
    try:
        ctx.set_option("cf_lds_max_pairs", 0)
        g0 = base.dev.x2i_recall(trig, pref, 200)
        e0 = base.dev.x2i_recall(edge, epref, 6000)
    finally:
        ctx.set_option("cf_lds_max_pairs", cases.KNOB_DEFAULT)
    g1 = base.dev.x2i_recall(trig, pref, 200)
    e1 = base.dev.x2i_recall(edge, epref, 6000)
    assert_same(g0, want)
    assert_same(g1, g0)
    assert_same(e0, ewant)
    assert_same(e1, e0)


# ---- limits and errors ---------------------------------------------------------------------------------------------------------------

def test_distinct_x_limit(base):
    rng = np.random.default_rng(40)
    many = list(range(cases.R_MANY, cases.R_MANY + 17))
    pref = cases.wide_prefer(rng, 17)
    got = base.check([many[:16]], [pref[:16]], 4000)               # exactly 1 024 distinct X are served
    assert len(ref.hop1(base.host, many[:16], pref[:16])) == 1024 and got[2][0] > 2000
    others = [[cases.R_WIDE], many, many[:16], [cases.R_DYADIC]]
    opref = [[1.0], pref, pref[:16], [2.0]]
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall(others, opref, 300)
    assert e.value.code == -4 and "request 1 " in str(e.value) and "distinct X" in str(e.value)
    want = ref.x2i_recall(base.host, others, opref, 300)
    assert want[2][1] == 0
    assert_same(base.dev.last, want)                               # the other requests' outputs are written, the refused one answers 0
    base.check([[cases.R_WIDE], many[:3]], [[1.0], pref[:3]], 300)  # the next call on the context succeeds


def test_pair_limit(base):
    rng = np.random.default_rng(41)
    full = list(range(cases.R_LONG, cases.R_LONG + 64))
    assert pairs_of(base, full) == ref.MAX_PAIRS
    pref = cases.wide_prefer(rng, 65)
    base.check([full], [pref[:64]], 300)                           # 65 536 pairs are served
    over = full + [cases.R_ONE]
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([[cases.R_WIDE], [], over, over], [[1.0], [], pref, pref], 300)
    assert e.value.code == -4 and "request 2 " in str(e.value) and "pairs" in str(e.value)
    assert_same(base.dev.last, ref.x2i_recall(base.host, [[cases.R_WIDE], [], over, over], [[1.0], [], pref, pref], 300))
    base.check([[cases.R_WIDE], full[:3]], [[1.0], pref[:3]], 300)


def test_argument_limits(base):
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([np.zeros(257, np.uint32)], [np.ones(257)], 10)
    assert e.value.code == -4
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([[70]], [[np.nan]], 10)
    assert e.value.code == -1
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([[70]], [[1.0]], 16385)
    assert e.value.code == -4
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([[70]] * 257, [[1.0]] * 257, 10)
    assert e.value.code == -1


def test_upload_refusals_leave_the_table_unchanged(ctx, base):
    rng = np.random.default_rng(42)
    p = Pair(ctx, base.dev.table, ROWS, 100, ROW_OFFSET)
    try:
        p.upload_item2x(*cases.csr([rng.choice(100, n, replace=False) for n in (5, 64, 0, 3, 1, 17, 2, 2, 9, 30)]), 0)
        lens = (5, 64, 0, 1024, 17, 3, 1, 65, 63, 9)
        p.upload_x2item(*cases.csr([rng.choice(ROWS, n, replace=False) for n in lens], [rng.standard_normal(n) for n in lens]), 0)
        trig, pref = [list(range(10)), [3]], [cases.wide_prefer(rng, 10), [2.0]]
        before = p.check(trig, pref, 1500)
        info = p.dev.info()
        assert info["rows"] == ROWS and info["n_x"] == 100 and info["i2x_pairs"] == 133 and info["x2i_pairs"] == sum(lens)
        one = np.ones(3, np.float32)
        bad_x = [
            cases.csr([np.arange(1025)], [np.ones(1025)]),                        # an X's item list longer than 1 024
            cases.csr([[1, 2, 3], [4, ROWS, 5]], [one, one]),                      # an item row >= rows
            cases.csr([[1, 2, 3]], [[1.0, np.inf, 1.0]]),                          # a non-finite score
            cases.csr([[1, 2, 3]], [[np.nan, 1.0, 1.0]]),
            cases.csr([[1, 2, 3], [9, 8, 9]], [one, one]),                         # an item twice in one list
            (np.array([0, 3, 2], np.uint64), np.arange(3, dtype=np.uint32), one),  # offsets that descend
        ]
        bad_i = [
            cases.csr([np.arange(50), np.arange(65)]),                             # an item's X list longer than 64
            cases.csr([[1, 2], [3, 100]]),                                         # an x id >= n_x
            cases.csr([[1, 2], [7, 3, 7]]),                                        # an x id twice in one list
        ]
        for bad, up, at in ((bad_x, p.dev.upload_x2item, 10), (bad_i, p.dev.upload_item2x, 10)):
            for args in bad:
                with pytest.raises(PgError) as e:
                    up(*args, at)
                assert e.value.code == -1
                assert p.dev.info() == info
                assert_same(p.dev.x2i_recall(trig, pref, 1500), before)
        for up, args in ((p.dev.upload_x2item, cases.csr([[1]], [[1.0]])), (p.dev.upload_item2x, cases.csr([[1]]))):
            with pytest.raises(PgError) as e:                                      # keys arrive in ascending order
                up(*args, 4)
            assert e.value.code == -1
        with pytest.raises(PgError):
            p.dev.upload_x2item(*cases.csr([[1]], [[1.0]]), 100)                    # outside the table's X
        assert_same(p.dev.x2i_recall(trig, pref, 1500), before)
        p.upload_x2item(*cases.csr([[1, 2, 3]], [one]), 11)                        # ... and good uploads still land (X 10, row 10 stay empty)
        p.upload_item2x(*cases.csr([[11, 1]]), 11)
        assert p.dev.info()["x2i_pairs"] == info["x2i_pairs"] + 3 and p.dev.info()["i2x_pairs"] == info["i2x_pairs"] + 2
        p.check(trig + [[11, 10]], pref + [[1.0, 2.0]], 1500)
    finally:
        p.dev.destroy()


def test_create_refusals(ctx, base):
    for n_x in (0, U32MAX):
        with pytest.raises(PgError) as e:
            pa.XTable(ctx, base.dev.table, n_x)
        assert e.value.code == -1


def test_generation_swap_makes_the_table_stale(ctx):
    t1, t2 = pa.Table(ctx, 300, DIM, 5), pa.Table(ctx, 300, DIM, 9)
    p = Pair(ctx, t1, 300, 4, 5)
    try:
        p.upload_item2x(*cases.csr([[1, 2], [2]]), 0)
        p.upload_x2item(*cases.csr([[1, 2, 3], [3, 4]], [[0.5, 0.25, 1.0], [1.0, 2.0]]), 1)
        p.check([[0, 1]], [[1.0, 3.0]], 8)
        t1.swap(t2)
        with pytest.raises(PgError) as e:
            p.dev.x2i_recall([[0, 1]], [[1.0, 3.0]], 8)
        assert e.value.code == -1 and "generation" in str(e.value)
    finally:
        p.dev.destroy()
        t1.destroy()
        t2.destroy()


# ---- exclusion ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_rule", [False, True])
def test_exclusion_lists(base, max_rule):
    rng = np.random.default_rng(51)
    trig = [rng.integers(0, 60000, 25) for _ in range(5)]
    pref = [cases.wide_prefer(rng, 25) for _ in range(5)]
    plain = ref.x2i_recall(base.host, trig, pref, 9000, True, max_rule)
    assert plain[2].min() > 400
    cand = [plain[0][q][:plain[2][q]] for q in range(5)]
    all_ids = np.arange(ROW_OFFSET, ROW_OFFSET + ROWS, dtype=np.uint64)
    not_cand = np.setdiff1d(all_ids, cand[2])
    lists = [
        np.zeros(0, np.uint64),                                                    # empty
        cand[1][:300].copy(),                                                      # the whole head
        np.concatenate([not_cand[:50], np.array([ref.U64MAX, 3, ROW_OFFSET + ROWS + 1], dtype=np.uint64)]),   # ids that are no candidates
        rng.choice(all_ids, 4096, replace=False),                                  # 4 096 ids
        np.concatenate([cand[4][::2], cand[4][:7]]).astype(np.uint64)[:4096],      # every other candidate, some twice
    ]
    for k in (1, 200):
        got = base.check(trig, pref, k, True, max_rule, lists)
        assert np.array_equal(got[0][0], plain[0][0][:k])
        assert got[0][1][0] == cand[1][300]
    base.check(trig, pref, 12000, True, max_rule, lists)                           # deeper than any answer: padding behind the kept entries


def test_exclusion_depth_limit(base):
    lists = [np.arange(4096, dtype=np.uint64)]
    base.check([[70]], [[1.0]], 16384 - 4096, True, False, lists)
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([[70]], [[1.0]], 16384 - 4095, True, False, lists)
    assert e.value.code == -4
    with pytest.raises(PgError) as e:
        base.dev.x2i_recall([[70]], [[1.0]], 10, True, False, [np.arange(4097, dtype=np.uint64)])
    assert e.value.code == -4


# ---- device buffers ------------------------------------------------------------------------------------------------------------------

def recall_dev(ctx, base, trig, pref, k, normalize, max_rule, lists):
    nq = len(trig)
    off = np.zeros(nq + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in trig])
    bufs = [ctx.to_device(np.concatenate(trig).astype(np.uint32)), ctx.to_device(np.concatenate(pref).astype(np.float64)),
            ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 8)]
    try:
        d_excl, xoff = 0, None
        if lists is not None:
            xoff = np.zeros(nq + 1, np.uint32)
            xoff[1:] = np.cumsum([len(l) for l in lists])
            bufs.append(ctx.to_device(np.concatenate(lists).astype(np.uint64)))
            d_excl = bufs[-1]
        counts = base.dev.x2i_recall_dev(bufs[0], bufs[1], off, k, bufs[2], bufs[3], normalize, max_rule, d_excl, xoff)
        rows, scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
        ctx.d2h(rows, bufs[2])
        ctx.d2h(scores, bufs[3])
    finally:
        for b in bufs:
            ctx.free(b)
    return rows, scores, counts


@pytest.mark.parametrize("with_lists", [False, True])
@pytest.mark.parametrize("max_rule", [False, True])
def test_dev_variant_equals_the_host_call(ctx, base, with_lists, max_rule):
    rng = np.random.default_rng(61)
    trig = [rng.integers(0, 60000, n) for n in (9, 0, 40)]
    pref = [cases.wide_prefer(rng, len(t)) for t in trig]
    all_ids = np.arange(ROW_OFFSET, ROW_OFFSET + ROWS, dtype=np.uint64)
    lists = [rng.choice(all_ids, n, replace=False) for n in (100, 5, 900)] if with_lists else None
    want = base.check(trig, pref, 333, True, max_rule, lists)
    assert_same(recall_dev(ctx, base, trig, pref, 333, True, max_rule, lists), want)


# ---- RealTimeU2I chained ---------------------------------------------------------------------------------------------------------------------

NAMES = ["click", "like", "play", "buy"]


@pytest.mark.parametrize("weight_mode", ["sum", "max"])
def test_rtu2i_x_recall_equals_triggers_then_x2i(ctx, base, weight_mode):
    rng = np.random.default_rng(71)
    conf = pa.RtU2I(rtu2i_cases.DECAY, NAMES, event_weight="click:1;like:2.5;buy:-3", event_play_time="play:5;like:30", weight_mode=weight_mode,
                    trigger_count=40, limit=1000)
    try:
        nq, k = 24, 300
        ev = list(rtu2i_cases.random_batch(rng, nq, 60000, len(NAMES)))
        for a in ev[:4]:
            a[3] = a[3][:0]                                                        # a request without events
        ev[0][5][:] = np.resize(np.arange(cases.R_SHARED, cases.R_SHARED + 256, dtype=np.uint32), len(ev[0][5]))   # ... and one over the shared X
        t_rows, t_w, t_cnt = conf.triggers(ctx, ROWS, *ev)
        trig = [t_rows[q][:t_cnt[q]] for q in range(nq)]
        pref = [t_w[q][:t_cnt[q]] for q in range(nq)]
        assert t_cnt[3] == 0 and t_cnt.max() == 40
        want = base.check(trig, pref, k, False, True)
        assert want[2][3] == 0 and want[2].max() == k
        assert_same(base.dev.rtu2i_x_recall(conf, *ev, k), want)                   # host arrays
        er, ec, ep, et, off, nw = pa.engine._pack_events(*ev)
        bufs = [ctx.to_device(er), ctx.to_device(ec), ctx.to_device(ep), ctx.to_device(et), ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 8)]
        try:
            counts = base.dev.rtu2i_x_recall_dev(conf, bufs[0], bufs[1], bufs[2], bufs[3], off, nw, k, bufs[4], bufs[5])
            rows, scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
            ctx.d2h(rows, bufs[4])
            ctx.d2h(scores, bufs[5])
        finally:
            for b in bufs:
                ctx.free(b)
        assert_same((rows, scores, counts), want)                                  # device arrays: no host read-back between the kernels
        lists = [want[0][q][:5].copy() for q in range(nq)]
        assert_same(base.dev.rtu2i_x_recall(conf, *ev, 100, lists), base.check(trig, pref, 100, False, True, lists))
    finally:
        conf.free()


# ---- into the fan-in ---------------------------------------------------------------------------------------------------------------------------

def test_dev_outputs_feed_the_fanin_merge(ctx, base):
    rng = np.random.default_rng(81)
    nq, k_x, k_cf = 6, 120, 80
    sim = pa.SimTable(ctx, base.dev.table)
    sim_host = cf_ref.SimLists(ROWS, ROW_OFFSET)
    bufs = []
    try:
        off = np.arange(401, dtype=np.uint64) * np.uint64(60)
        nb = np.concatenate([rng.choice(62100, 60, replace=False) for _ in range(400)]).astype(np.uint32)
        sm = rng.uniform(0.05, 1.0, nb.size).astype(np.float32)
        sim.upload(off, nb, sm, 0)
        sim_host.upload(off, nb, sm, 0)
        trig = [rng.choice(400, 12, replace=False).astype(np.uint32) for _ in range(nq)]
        trig[2] = np.zeros(0, np.uint32)                                           # a request only the other recall answers
        pref = [rng.uniform(0.1, 3.0, len(t)) for t in trig]
        x_trig = [np.concatenate([t, [cases.R_FAN + q, cases.R_DYADIC]]).astype(np.uint32) for q, t in enumerate(trig)]
        x_pref = [np.concatenate([p, [1.5, 2.0]]) for p in pref]
        want_x = ref.x2i_recall(base.host, x_trig, x_pref, k_x, True)
        want_cf = cf_ref.cf_recall(sim_host, trig, pref, k_cf, True)
        want = fanin_ref.merge([(want_x[0], want_x[1]), (want_cf[0], want_cf[1])])
        toff = np.zeros(nq + 1, np.uint32)
        toff[1:] = np.cumsum([len(t) for t in trig])
        xoff = np.zeros(nq + 1, np.uint32)
        xoff[1:] = np.cumsum([len(t) for t in x_trig])
        d_tr, d_pf = ctx.to_device(np.concatenate(trig)), ctx.to_device(np.concatenate(pref))
        d_xt, d_xp = ctx.to_device(np.concatenate(x_trig)), ctx.to_device(np.concatenate(x_pref))
        d_xr, d_xs, d_cr, d_cs = ctx.malloc(nq * k_x * 8), ctx.malloc(nq * k_x * 8), ctx.malloc(nq * k_cf * 8), ctx.malloc(nq * k_cf * 8)
        bufs += [d_tr, d_pf, d_xt, d_xp, d_xr, d_xs, d_cr, d_cs]
        base.dev.x2i_recall_dev(d_xt, d_xp, xoff, k_x, d_xr, d_xs, True)
        sim.cf_recall_dev(d_tr, d_pf, toff, k_cf, d_cr, d_cs, True)
        cap = k_x + k_cf
        outs = [np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.float64), np.empty((nq, cap), np.uint8),
                np.empty((2, nq, cap), np.float64), np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)]
        d_out = [ctx.malloc(a.nbytes) for a in outs]
        bufs += d_out
        ctx.fanin_merge_dev([(d_xr, d_xs, k_x, True), (d_cr, d_cs, k_cf, True)], nq, *d_out)
        ctx.synchronize()
        for a, p in zip(outs, d_out):
            ctx.d2h(a, p)
        fanin_ref.same(tuple(outs), want)
        assert np.all(outs[5] > 0)
    finally:
        for b in bufs:
            ctx.free(b)
        sim.destroy()
