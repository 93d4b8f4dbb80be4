"""GPU tests of RealTimeU2IRecall on the device (csrc/rtu2i.hip, csrc/cf.hip): the trigger kernel against the
host statement, the max-rule expansion against tests/rtu2i_ref.py, the one-call recall against the two in sequence.  Ids, counts
and the fp64 BITS of weights and scores must be equal.  The base similarity table is over an item table of 5 000 x 64 rows with
a nonzero row_offset whose lists have 0, 1, 63, 64, 65 or 1 024 entries; a small second one carries the crafted lists."""
import numpy as np
import pytest

import pairec_amd as pa
import rtu2i_cases as cases
import rtu2i_ref as ref
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

ROWS, DIM, ROW_OFFSET = 5000, 64, 1 << 20
LDS_MAX_PAIRS, MAX_PAIRS = 6144, 65536            # cf.hip: the LDS tier's default limit, the call's limit
TRIG_SLOTS = 2048                                 # rtu2i.hip: the trigger kernel's item table ...
HASH_MUL = 0x9E3779B1                             # ... and its hash: ((row * HASH_MUL mod 2^32) * slots) >> 32
U32MAX = 0xFFFFFFFF
BIG = 1 << 22                                     # an item-table size for the trigger stage alone (it reads no table)
NAMES = ["click", "like", "play", "buy"]


def slot(rows, slots):
    return ((np.asarray(rows, np.uint64) * np.uint64(HASH_MUL) & np.uint64(U32MAX)) * np.uint64(slots)) >> np.uint64(32)


def same(got, want):
    assert np.array_equal(np.asarray(got[2], np.uint32), np.asarray(want[2], np.uint32))
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))


def wide_ints(rng, n):
    """event times that are weights under "eventTime / 1": magnitudes from 1 to 1e17, mixed signs — any other addition order
    changes bits"""
    return (10.0 ** rng.uniform(0, 17, n) * rng.choice([-1.0, 1.0], n)).astype(np.int64)


def wide_prefer(rng, n):
    return 10.0 ** rng.uniform(-8, 16, n) * rng.choice([-1.0, 1.0], n)


def csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l[0]) for l in lists])
    nb = np.concatenate([np.asarray(l[0], np.uint32) for l in lists]) if lists else np.zeros(0, np.uint32)
    sm = np.concatenate([np.asarray(l[1], np.float32) for l in lists]) if lists else np.zeros(0, np.float32)
    return off, nb, sm


class Pair:
    """a device similarity table and its host restatement, uploaded together"""

    def __init__(self, ctx, rows, row_offset, lists):
        self.table = pa.Table(ctx, rows, DIM, row_offset)
        self.dev = pa.SimTable(ctx, self.table)
        self.host = ref.SimLists(rows, row_offset)
        off, nb, sm = csr(lists)
        self.dev.upload(off, nb, sm, 0)
        self.host.upload(off, nb, sm, 0)
        self.lens = np.array([len(l[0]) for l in lists])

    def check(self, trig, pref, k, lists=None):
        got = self.dev.rtu2i_expand(trig, pref, k, lists)
        same(got, ref.expand(self.host, trig, pref, k, lists))
        return got

    def destroy(self):
        self.dev.destroy()
        self.table.destroy()


@pytest.fixture(scope="module")
def base(ctx):
    rng = np.random.default_rng(11)
    lens = rng.choice([0, 1, 63, 64, 65, 1024], ROWS, p=[0.15, 0.2, 0.2, 0.2, 0.2, 0.05])
    lens[0:70], lens[70:90], lens[90:100], lens[100:110], lens[110:120] = 1024, 64, 63, 1, 65
    p = Pair(ctx, ROWS, ROW_OFFSET, [(rng.choice(ROWS, n, replace=False), rng.standard_normal(n).astype(np.float32)) for n in lens])
    yield p
    p.destroy()


@pytest.fixture(scope="module")
def crafted(ctx):
    rng = np.random.default_rng(13)
    lists = []
    shared = np.arange(1000, 1050)
    for _ in range(256):                              # rows 0 .. 255: the same 50 neighbours, each in an order of its own
        lists.append((rng.permutation(shared), rng.uniform(0.1, 1.0, 50).astype(np.float32)))
    for _ in range(8):                                # rows 256 .. 263: dyadic similarities over 20 neighbours
        lists.append((1100 + rng.permutation(20), rng.choice([0.25, 0.5, 0.75, 1.0], 20).astype(np.float32)))
    lists.append(([1200, 1201], [0.0, 1.0]))          # rows 264, 265: a similarity of zero
    lists.append(([1200, 1201], [0.0, 2.0]))
    p = Pair(ctx, 2000, 7, lists)
    yield p
    p.destroy()


@pytest.fixture(scope="module")
def confs():
    c = {
        "sum": pa.RtU2I("eventTime / 1", weight_mode="sum", limit=256),          # an event's weight is its time
        "max": pa.RtU2I("eventTime / 1", weight_mode="max", limit=256),
        "decay": pa.RtU2I(cases.DECAY, NAMES, event_weight="click:1;like:2.5;buy:-3", event_play_time="play:5;like:30", trigger_count=40, limit=1000),
        "decay_max": pa.RtU2I(cases.DECAY, NAMES, event_weight="click:1;like:2.5;buy:-3", event_play_time="play:5;like:30", weight_mode="max",
                              trigger_count=200, limit=1000),
    }
    yield c
    for v in c.values():
        v.free()


def triggers_same(ctx, conf, table_rows, rows, codes, pt, times, now):
    want = conf.triggers_host(table_rows, rows, codes, pt, times, now)
    got = conf.triggers(ctx, table_rows, rows, codes, pt, times, now)
    same(got, want)
    return got


# ---- the trigger kernel ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["sum", "max"])
def test_event_counts_at_the_wave_and_block_edges(ctx, confs, mode):
    rng = np.random.default_rng(21)
    ns = [0, 1, 63, 64, 65, 1023, 1024]
    rows = [rng.integers(0, 300, n) for n in ns]                                # ~3 events per item in the long requests
    got = triggers_same(ctx, confs[mode], BIG, rows, [np.zeros(n, np.uint16) for n in ns], None, [wide_ints(rng, n) for n in ns], [0] * len(ns))
    assert got[2][0] == 0 and got[2][1] == 1 and got[2][6] == 256


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_1024_events_of_one_item(ctx, confs, mode):
    rng = np.random.default_rng(22)
    times = wide_ints(rng, 1024)
    got = triggers_same(ctx, confs[mode], BIG, [np.full(1024, 77)], [np.zeros(1024, np.uint16)], None, [times], [0])
    assert got[2][0] == 1 and got[0][0, 0] == 77
    if mode == "max":
        assert got[1][0, 0] == float(times.max())
    else:                                                                       # ... and the sum depends on the order
        back = confs[mode].triggers_host(BIG, [np.full(1024, 77)], [np.zeros(1024, np.uint16)], None, [times[::-1]], [0])
        assert back[1][0, 0] != got[1][0, 0]


def test_1024_distinct_items(ctx, confs):
    rng = np.random.default_rng(23)
    rows = rng.permutation(BIG)[:1024]
    times = rng.integers(-50, 50, 1024)                                         # many equal weights: the first index decides
    got = triggers_same(ctx, confs["sum"], BIG, [rows], [np.zeros(1024, np.uint16)], None, [times], [0])
    assert got[2][0] == 256
    w = got[1][0]
    assert np.sum(w[1:] == w[:-1]) > 100


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_rows_that_collide_in_the_kernels_hash(ctx, confs, mode):
    rng = np.random.default_rng(24)
    every = np.arange(BIG)
    s = slot(every, TRIG_SLOTS)
    one_slot = every[s == 5]                                                    # one slot: a probe run as long as the item count
    run = every[(s >= 2040)]                                                    # the table's last slots: the probe wraps around
    assert len(one_slot) >= 1024 and len(run) >= 1024
    mult = np.arange(1, 401) * TRIG_SLOTS                                       # multiples of the slot count
    rows = [one_slot[:1024], rng.choice(one_slot[:300], 1024), rng.choice(run[:600], 1024), rng.choice(mult, 1000)]
    times = [wide_ints(rng, len(r)) for r in rows]
    got = triggers_same(ctx, confs[mode], BIG, rows, [np.zeros(len(r), np.uint16) for r in rows], None, times, [0] * 4)
    assert list(got[2]) == [256] * 4


def test_exp_grid_on_the_device(ctx):
    # the test that fails if the device contracts a product and a sum of go_exp into one fma
    grid = cases.exp_grid()
    conf = {False: pa.RtU2I(cases.EXP_POS, limit=256), True: pa.RtU2I(cases.EXP_NEG, limit=256)}
    host = cases.run_exp_grid(grid, lambda neg, rows, codes, times, now: conf[neg].triggers_host(256, rows, codes, None, times, now))
    dev = cases.run_exp_grid(grid, lambda neg, rows, codes, times, now: conf[neg].triggers(ctx, 256, rows, codes, None, times, now))
    assert dev == host
    assert sum(g is not None for g in dev) > 10000
    for c in conf.values():
        c.free()


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(31)
    ev = cases.random_batch(rng, 256, ROWS, len(NAMES))
    for q in (3, 11, 19):                                                       # requests without events, and one of dropped events only
        for a in ev[:4]:
            a[q] = a[q][:0]
    ev[0][27][:] = ROWS + 1
    return ev


@pytest.mark.parametrize("name", ["decay", "decay_max"])
def test_mixed_batch_of_256_and_one_request_alone(ctx, confs, mixed, name):
    got = triggers_same(ctx, confs[name], ROWS, *mixed)
    assert got[2][3] == 0 and got[2][27] == 0 and got[2].max() == confs[name].trigger_count
    alone = confs[name].triggers(ctx, ROWS, *[a[7:8] for a in mixed])
    same(alone, tuple(g[7:8] for g in got))


def test_triggers_dev_on_device_buffers(ctx, confs, mixed):
    conf = confs["decay"]
    rows, codes, pt, times, now = [a[:9] for a in mixed]
    want = conf.triggers_host(ROWS, rows, codes, pt, times, now)
    er, ec, ep, et, off, nw = pa.engine._pack_events(rows, codes, pt, times, now)
    T, nq = conf.trigger_count, 9
    bufs = [ctx.to_device(er), ctx.to_device(ec), ctx.to_device(ep), ctx.to_device(et), ctx.malloc(nq * T * 4), ctx.malloc(nq * T * 8), ctx.malloc(nq * 4)]
    try:
        conf.triggers_dev(ctx, ROWS, bufs[0], bufs[1], bufs[2], bufs[3], off, nw, bufs[4], bufs[5], bufs[6])
        got = (np.empty((nq, T), np.uint32), np.empty((nq, T), np.float64), np.empty(nq, np.uint32))
        for a, b in zip(got, bufs[4:]):
            ctx.d2h(a, b)
    finally:
        for b in bufs:
            ctx.free(b)
    same(got, want)


# ---- the max-rule expansion ------------------------------------------------------------------------------------------------------------

def test_256_triggers_over_shared_neighbours(crafted):
    rng = np.random.default_rng(41)
    trig, pref = rng.permutation(256), wide_prefer(rng, 256)
    got = crafted.check([trig], [pref], 64)
    assert got[2][0] == 50
    summed = crafted.dev.cf_recall([trig], [pref], 64, normalize=False)
    assert not np.array_equal(summed[1], got[1])                                # not the sum


def test_first_of_equal_zeros_stays(crafted):
    got = crafted.check([[264, 265], [265, 264], [264, 265]], [[1.0, -1.0], [-1.0, 1.0], [-1.0, -2.0]], 4)
    z = got[1].view(np.uint64)
    assert got[0][0, 1] == 7 + 1200 and z[0, 1] == 0                            # 0.0, then -0.0: the first stays
    assert z[1, 0] == 0x8000000000000000 or z[1, 1] == 0x8000000000000000       # -0.0, then 0.0


def test_dyadic_similarities_tie_across_rows(crafted):
    trig = list(range(256, 264))
    got = crafted.check([trig, trig[:3]], [[1, 2, 4, 1, 2, 4, 1, 2], [2, 2, 4]], 20)
    sc = got[1][0]
    tie = np.nonzero(sc[1:] == sc[:-1])[0]
    assert len(tie) > 0 and np.all(got[0][0][tie] < got[0][0][tie + 1])


def test_k_edges(base):
    rng = np.random.default_rng(42)
    trig = [70, 71, 90, 100, 110]
    pref = wide_prefer(rng, len(trig))
    distinct = len(ref.accumulate_max(base.host, trig, pref))
    assert distinct > 100
    for k in (1, distinct, distinct + 1):
        assert base.check([trig], [pref], k)[2][0] == min(k, distinct)


def test_trigger_rows_beyond_the_table(base):
    rng = np.random.default_rng(43)
    trig = [[], [U32MAX], [ROWS, ROWS + 1, U32MAX - 1], [71, U32MAX, 90, ROWS, 71, 100], rng.integers(0, ROWS, 256)]
    got = base.check(trig, [wide_prefer(rng, len(t)) for t in trig], 300)
    assert list(got[2][:3]) == [0, 0, 0] and got[2][3] > 64


def test_exclusion_list(base):
    rng = np.random.default_rng(44)
    trig = [rng.integers(0, ROWS, 25) for _ in range(3)]
    pref = [wide_prefer(rng, 25) for _ in range(3)]
    plain = ref.expand(base.host, trig, pref, 5000)
    lists = [np.zeros(0, np.uint64), plain[0][1][:300].copy(), rng.choice(np.arange(ROW_OFFSET, ROW_OFFSET + ROWS, dtype=np.uint64), 4096, replace=False)]
    got = base.check(trig, pref, 200, lists)
    assert np.array_equal(got[0][0], plain[0][0][:200]) and got[0][1][0] == plain[0][1][300]


def rows_of_length(base, n, count):
    r = np.nonzero(base.lens == n)[0]
    assert len(r) >= count
    return [int(x) for x in r[:count]]


def request_of_pairs(base, pairs):
    """triggers whose lists hold exactly `pairs` entries in all"""
    n1024, rest = divmod(pairs, 1024)
    n64, rest = divmod(rest, 64)
    n63 = 0
    if rest == 63:
        n63, rest = 1, 0
    trig = rows_of_length(base, 1024, n1024) + rows_of_length(base, 64, n64) + rows_of_length(base, 63, n63) + rows_of_length(base, 1, rest)
    assert sum(base.host.length(r) for r in trig) == pairs
    return trig


def test_both_tiers_give_one_answer(ctx, base):
    rng = np.random.default_rng(45)
    edge = [request_of_pairs(base, n) for n in (LDS_MAX_PAIRS - 1, LDS_MAX_PAIRS, LDS_MAX_PAIRS + 1)]
    pref = [wide_prefer(rng, len(t)) for t in edge]
    want = ref.expand(base.host, edge, pref, 5000)
    try:
        ctx.set_option("cf_lds_max_pairs", 0)
        g0 = base.dev.rtu2i_expand(edge, pref, 5000)
    finally:
        ctx.set_option("cf_lds_max_pairs", LDS_MAX_PAIRS)
    g1 = base.dev.rtu2i_expand(edge, pref, 5000)
    same(g0, want)
    same(g1, g0)


def test_expand_dev_on_device_buffers(ctx, base):
    rng = np.random.default_rng(46)
    trig = [rng.integers(0, ROWS, n) for n in (9, 0, 40)]
    pref = [wide_prefer(rng, len(t)) for t in trig]
    nq, k = 3, 333
    want = ref.expand(base.host, trig, pref, k)
    off = np.zeros(nq + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in trig])
    bufs = [ctx.to_device(np.concatenate(trig).astype(np.uint32)), ctx.to_device(np.concatenate(pref).astype(np.float64)),
            ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 8)]
    try:
        counts = base.dev.rtu2i_expand_dev(bufs[0], bufs[1], off, k, bufs[2], bufs[3])
        rows, scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
        ctx.d2h(rows, bufs[2])
        ctx.d2h(scores, bufs[3])
    finally:
        for b in bufs:
            ctx.free(b)
    same((rows, scores, counts), want)


# ---- the recall ------------------------------------------------------------------------------------------------------------------------

def recall_want(conf, base, ev, k, lists=None):
    """the host statement of the trigger stage, then the reference expansion of what it kept"""
    tr, tw, tc = conf.triggers_host(ROWS, *ev)
    nq = len(ev[0])
    return ref.expand(base.host, [tr[q, :tc[q]] for q in range(nq)], [tw[q, :tc[q]] for q in range(nq)], k, lists), tc


def recall_dev(ctx, conf, base, ev, k):
    er, ec, ep, et, off, nw = pa.engine._pack_events(*ev)
    nq = len(ev[0])
    bufs = [ctx.to_device(er), ctx.to_device(ec), ctx.to_device(ep), ctx.to_device(et), ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 8)]
    try:
        counts = base.dev.rtu2i_recall_dev(conf, bufs[0], bufs[1], bufs[2], bufs[3], off, nw, k, bufs[4], bufs[5])
        rows, scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
        ctx.d2h(rows, bufs[4])
        ctx.d2h(scores, bufs[5])
    finally:
        for b in bufs:
            ctx.free(b)
    return rows, scores, counts


@pytest.mark.parametrize("name", ["decay", "decay_max"])
def test_recall_equals_triggers_then_expansion(ctx, confs, base, mixed, name):
    ev = [a[:32] for a in mixed]
    rows_short = [r[r >= 120] for r in ev[0]]                                   # (keep the 1 024-entry lists of rows 0 .. 69 out: 65 536 pairs is the call's limit)
    keep = [r >= 120 for r in ev[0]]
    ev = [rows_short] + [[a[q][keep[q]] for q in range(32)] for a in ev[1:4]] + [ev[4]]
    want, tc = recall_want(confs[name], base, ev, 300)
    assert tc[3] == 0 and tc[27] == 0 and tc.max() == confs[name].trigger_count
    assert want[2][3] == 0 and want[2].max() == 300
    same(recall_dev(ctx, confs[name], base, ev, 300), want)
    same(base.dev.rtu2i_recall(confs[name], *ev, 300), want)                    # host arrays: the same call behind a staging copy
    lists = [want[0][q][:5].copy() for q in range(32)]
    want_x, _ = recall_want(confs[name], base, ev, 100, lists)
    same(base.dev.rtu2i_recall(confs[name], *ev, 100, lists), want_x)


def test_recall_reports_a_request_over_the_pair_limit(ctx, confs, base):
    # 65 triggers with lists of 1 024 entries: 66 560 pairs
    rng = np.random.default_rng(51)
    over = np.arange(65, dtype=np.uint32)
    ev = ([np.array([200, 201]), over], [np.zeros(2, np.uint16), np.zeros(65, np.uint16)], None,
          [wide_ints(rng, 2), np.arange(1, 66)], [0, 0])
    with pytest.raises(PgError) as e:
        base.dev.rtu2i_recall(confs["sum"], *ev, 300)
    assert e.value.code == -4 and "request 1" in str(e.value)
    ok = ([np.array([200, 201]), over[:64]], ev[1][:1] + [np.zeros(64, np.uint16)], None, [ev[3][0], np.arange(1, 65)], [0, 0])
    want, _ = recall_want(confs["sum"], base, ok, 300)
    same(base.dev.rtu2i_recall(confs["sum"], *ok, 300), want)                   # 65 536 pairs are served, on the same context


def test_recall_refuses_1025_events(ctx, confs, base):
    big = np.full(1025, 200, np.uint32)
    ev = ([np.array([200]), big], [np.zeros(1, np.uint16), np.zeros(1025, np.uint16)], None, [np.array([5]), np.arange(1025)], [0, 0])
    with pytest.raises(PgError) as e:
        base.dev.rtu2i_recall(confs["sum"], *ev, 50)
    assert e.value.code == -4 and "request 1" in str(e.value)
    ok = [a[:1] if a is not None else None for a in ev[:4]] + [[0]]
    want, _ = recall_want(confs["sum"], base, ok, 50)
    same(base.dev.rtu2i_recall(confs["sum"], *ok, 50), want)
