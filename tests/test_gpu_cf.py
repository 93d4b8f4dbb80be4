"""GPU tests of the collaborative-filter recall (csrc/cf.hip) against tests/cf_ref.py: ids, fp64 score BITS,
counts and padding must be equal.  The base case is an item table of 5 000 x 64 rows with a nonzero row_offset whose lists have
0, 1, 63, 64, 65 or 1 024 entries and a band of rows never uploaded; a second, larger item table carries the crafted lists
(shared neighbours, rows that collide in the kernel's hash, dyadic similarities)."""
import numpy as np
import pytest

import cf_ref as ref
import pairec_amd as pa
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

ROWS, DIM, ROW_OFFSET = 5000, 64, 1 << 20
BAND = (4000, 4500)                               # never uploaded
LDS_SLOTS, LDS_MAX_PAIRS, MAX_PAIRS = 12288, 6144, 65536      # cf.hip: the LDS tier's table, its default limit, the call's limit
HASH_MUL = 0x9E3779B1                             # ... and its hash: ((row * HASH_MUL mod 2^32) * slots) >> 32
U32MAX = 0xFFFFFFFF
BIG_ROWS = 16 * LDS_SLOTS + 1


def slot(rows, slots):
    return ((np.asarray(rows, np.uint64) * np.uint64(HASH_MUL) & np.uint64(U32MAX)) * np.uint64(slots)) >> np.uint64(32)


def assert_same(got, want):
    assert np.array_equal(np.asarray(got[2], np.uint32), np.asarray(want[2], np.uint32))
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))


def csr(lists):
    """[(neighbours, similarities)] per row → offsets, neighbours, similarities"""
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l[0]) for l in lists])
    nb = np.concatenate([np.asarray(l[0], np.uint32) for l in lists]) if lists else np.zeros(0, np.uint32)
    sm = np.concatenate([np.asarray(l[1], np.float32) for l in lists]) if lists else np.zeros(0, np.float32)
    return off, nb, sm


class Pair:
    """a device similarity table and its host restatement, uploaded together"""

    def __init__(self, ctx, table, rows, row_offset):
        self.dev = pa.SimTable(ctx, table)
        self.host = ref.SimLists(rows, row_offset)

    def upload(self, lists, row0):
        off, nb, sm = csr(lists)
        self.dev.upload(off, nb, sm, row0)
        self.host.upload(off, nb, sm, row0)

    def check(self, triggers, prefer, k, normalize=True, lists=None):
        got = self.dev.cf_recall(triggers, prefer, k, normalize, lists)
        assert_same(got, ref.cf_recall(self.host, triggers, prefer, k, normalize, lists))
        return got


def base_lengths():
    rng = np.random.default_rng(11)
    lens = rng.choice([0, 1, 63, 64, 65, 1024], ROWS, p=[0.15, 0.2, 0.2, 0.2, 0.2, 0.05])
    lens[0:70], lens[70:90], lens[90:100], lens[100:110], lens[110:120] = 1024, 64, 63, 1, 65
    return lens


@pytest.fixture(scope="module")
def base(ctx):
    rng = np.random.default_rng(12)
    t = pa.Table(ctx, ROWS, DIM, ROW_OFFSET)
    p = Pair(ctx, t, ROWS, ROW_OFFSET)
    lens = base_lengths()
    lists = [(rng.choice(ROWS, n, replace=False), rng.standard_normal(n).astype(np.float32)) for n in lens]
    p.upload(lists[:BAND[0]], 0)
    p.upload(lists[BAND[1]:], BAND[1])               # (the rows in between keep empty lists)
    p.lens = lens
    yield p
    p.dev.destroy()
    t.destroy()


@pytest.fixture(scope="module")
def crafted(ctx):
    rng = np.random.default_rng(13)
    t = pa.Table(ctx, BIG_ROWS, DIM, 7)
    p = Pair(ctx, t, BIG_ROWS, 7)
    every = np.arange(BIG_ROWS)
    lists = []
    shared = np.arange(1000, 1050)
    for _ in range(256):                              # rows 0 .. 255: the same 50 neighbours, each in an order of its own
        lists.append((rng.permutation(shared), rng.uniform(0.1, 1.0, 50).astype(np.float32)))
    collide = [
        np.arange(1, 16) * LDS_SLOTS,                 # 256: multiples of the LDS tier's slot count
        7 + 1024 * np.arange(150),                    # 257: equal low bits
        2048 * np.arange(1, 91),                      # 258: multiples of a global-tier slot count
        every[(slot(every, LDS_SLOTS) >= 100) & (slot(every, LDS_SLOTS) < 150)][:1024],   # 259: one long probe run in the LDS table
        every[slot(every, 1024) == 5][:1024],         # 260: one slot of the smallest global table, neighbours in every larger one
    ]
    for nb in collide:
        lists.append((nb, rng.standard_normal(len(nb)).astype(np.float32)))
    for _ in range(8):                                # rows 261 .. 268: dyadic similarities over 20 neighbours
        lists.append((5000 + rng.permutation(20), rng.choice([0.25, 0.5, 0.75, 1.0], 20).astype(np.float32)))
    p.upload(lists, 0)
    p.collide_lens = [len(nb) for nb in collide]
    yield p
    p.dev.destroy()
    t.destroy()


def wide_prefer(rng, n):
    """magnitudes from 1e-8 to 1e16, mixed signs: any other addition order changes bits"""
    return 10.0 ** rng.uniform(-8, 16, n) * rng.choice([-1.0, 1.0], n)


# ---- accumulation and ordering -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
def test_shared_neighbours_256_ordered_additions(crafted, normalize):
    rng = np.random.default_rng(21)
    trig = rng.permutation(256)
    got = crafted.check([trig], [wide_prefer(rng, 256)], 64, normalize)
    assert got[2][0] == 50


def test_addition_order_on_the_device(crafted):
    # 1e16 + s - 1e16 per item: everything below 1e16's last place is lost, in this order only
    crafted.check([[0, 1, 2], [0, 2, 1]], [[1e16, 1.0, -1e16], [1e16, -1e16, 1.0]], 50, False)


@pytest.mark.parametrize("lds_max_pairs", [0, LDS_MAX_PAIRS])
def test_colliding_rows(ctx, crafted, lds_max_pairs):
    rng = np.random.default_rng(22)
    trig = [[256, 257, 258], [259], [260], [260, 259, 258, 257, 256, 259]]
    pref = [wide_prefer(rng, len(t)) for t in trig]
    try:
        ctx.set_option("cf_lds_max_pairs", lds_max_pairs)
        got = crafted.check(trig, pref, 2048, True)
    finally:
        ctx.set_option("cf_lds_max_pairs", LDS_MAX_PAIRS)
    assert got[2][1] == crafted.collide_lens[3] and got[2][2] == crafted.collide_lens[4]


@pytest.mark.parametrize("normalize", [False, True])
def test_ties_in_row_order(crafted, normalize):
    trig = list(range(261, 269))
    got = crafted.check([trig, trig[:3]], [[1, 2, 3, 4, 1, 2, 3, 4], [2, 2, 4]], 20, normalize)
    sc = got[1][0]
    assert np.sum(sc[1:] == sc[:-1]) > 0                       # equal sums across different rows
    tie = np.nonzero(sc[1:] == sc[:-1])[0]
    assert np.all(got[0][0][tie] < got[0][0][tie + 1])


def test_negative_preferences_are_not_divided(crafted):
    rng = np.random.default_rng(23)
    trig = rng.permutation(256)[:40]
    pref = -np.abs(wide_prefer(rng, 40))
    got = crafted.check([trig], [pref], 50, True)              # every score negative: m stays 0
    assert_same(got, crafted.dev.cf_recall([trig], [pref], 50, False))
    assert np.all(got[1][0] < 0)
    # a similarity of zero under a negative preference: -0.0, ranked as 0.0, its bits kept
    crafted.check([[261, 0]], [[-0.0, -1.0]], 70, True)


def test_k_edges(base):
    rng = np.random.default_rng(24)
    trig = [70, 71, 90, 100, 110]
    pref = wide_prefer(rng, len(trig))
    distinct = len(ref.accumulate(base.host, trig, pref))
    assert distinct > 100
    for k in (1, distinct, distinct + 1, distinct + 777):
        got = base.check([trig], [pref], k)
        assert got[2][0] == min(k, distinct)


def test_trigger_edges(base):
    rng = np.random.default_rng(25)
    band = BAND[0] + 5
    assert base.host.length(band) == 0
    trig = [
        [],                                                     # no triggers: count 0
        [U32MAX],
        [ROWS, ROWS + 1, U32MAX - 1],                           # >= rows
        [band],                                                 # never uploaded
        [70],
        [70, 70],                                               # a trigger twice contributes twice
        [71, U32MAX, 90, ROWS, 71, band, 100],
        rng.integers(0, ROWS, 256),                             # 256 triggers
        [int(np.nonzero(base.lens == 0)[0][0])],                # an empty list
    ]
    pref = [wide_prefer(rng, len(t)) for t in trig]
    got = base.check(trig, pref, 300)
    assert list(got[2][:4]) == [0, 0, 0, 0] and got[2][8] == 0
    assert got[2][4] == 64 and got[2][5] == 64
    # the trigger items themselves stay in the answer
    self_row = 120
    nb = base.host.lists[self_row][0]
    if nb:
        t2 = [self_row, nb[0]]
        base.check([t2], [[1.0, 1.0]], 2000)


# ---- batching and tiers --------------------------------------------------------------------------------------------------------------

def rows_of_length(base, n, count, start=0):
    r = np.nonzero(base.lens == n)[0]
    r = r[(r < BAND[0]) | (r >= BAND[1])]
    assert len(r) >= start + count
    return [int(x) for x in r[start:start + count]]


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


@pytest.fixture(scope="module")
def mixed(base):
    rng = np.random.default_rng(31)
    trig = []
    for q in range(256):
        n = 0 if q % 8 == 3 else int(rng.integers(1, 30))
        if q in (40, 200):
            n = 256
        trig.append(rng.integers(0, ROWS + 50, n))            # (a few beyond the table)
    trig[7] = rng.integers(0, ROWS, 12)
    pref = [wide_prefer(rng, len(t)) for t in trig]
    want = ref.cf_recall(base.host, trig, pref, 200, True)
    return trig, pref, want


def test_mixed_batch_of_256(base, mixed):
    trig, pref, want = mixed
    assert_same(base.dev.cf_recall(trig, pref, 200), want)


def test_batching_invariance(base, mixed):
    trig, pref, want = mixed
    got = base.dev.cf_recall([trig[7]], [pref[7]], 200)
    assert_same(got, tuple(w[7:8] for w in want))


def test_both_tiers_give_one_answer(ctx, base, mixed):
    trig, pref, want = mixed
    rng = np.random.default_rng(32)
    # just under, at and just over the LDS tier's default limit
    edge = [request_of_pairs(base, n) for n in (LDS_MAX_PAIRS - 1, LDS_MAX_PAIRS, LDS_MAX_PAIRS + 1)]
    epref = [wide_prefer(rng, len(t)) for t in edge]
    ewant = ref.cf_recall(base.host, edge, epref, 5000, True)
    try:
        ctx.set_option("cf_lds_max_pairs", 0)
        g0 = base.dev.cf_recall(trig, pref, 200)
        e0 = base.dev.cf_recall(edge, epref, 5000)
    finally:
        ctx.set_option("cf_lds_max_pairs", LDS_MAX_PAIRS)
    g1 = base.dev.cf_recall(trig, pref, 200)
    e1 = base.dev.cf_recall(edge, epref, 5000)
    assert_same(g0, want)
    assert_same(g1, g0)
    assert_same(e0, ewant)
    assert_same(e1, e0)


# ---- limits and errors ---------------------------------------------------------------------------------------------------------------

def test_pair_limit(base):
    rng = np.random.default_rng(41)
    full = request_of_pairs(base, MAX_PAIRS)
    assert len(full) == 64
    pref = wide_prefer(rng, 65)
    base.check([full], [pref[:64]], 300)                       # 65 536 pairs are served
    over = full + rows_of_length(base, 1, 1)
    with pytest.raises(PgError) as e:
        base.dev.cf_recall([[70], over], [[1.0], pref], 300)
    assert e.value.code == -4 and "request 1" in str(e.value)
    base.check([[70], full[:3]], [[1.0], pref[:3]], 300)       # the next call on the context succeeds


def test_argument_limits(base):
    with pytest.raises(PgError) as e:
        base.dev.cf_recall([np.zeros(257, np.uint32)], [np.ones(257)], 10)
    assert e.value.code == -4
    with pytest.raises(PgError) as e:
        base.dev.cf_recall([[70]], [[np.nan]], 10)
    assert e.value.code == -1
    with pytest.raises(PgError) as e:
        base.dev.cf_recall([[70]], [[1.0]], 16385)
    assert e.value.code == -4


def test_upload_refusals_leave_the_table_unchanged(ctx, base):
    rng = np.random.default_rng(42)
    t = base.dev.table
    p = Pair(ctx, t, ROWS, ROW_OFFSET)
    try:
        good = [(rng.choice(ROWS, n, replace=False), rng.standard_normal(n).astype(np.float32)) for n in (5, 64, 0, 1024, 17, 3, 1, 65, 63, 9)]
        p.upload(good, 0)
        trig, pref = [list(range(12)), [3]], [wide_prefer(rng, 12), [2.0]]
        before = p.check(trig, pref, 1500)
        info = p.dev.info()
        one = np.ones(3, np.float32)
        bad = [
            csr([(np.arange(1025), np.ones(1025, np.float32))]),                  # a list longer than 1 024
            csr([([1, 2, 3], one), ([4, ROWS, 5], one)]),                         # a neighbour >= rows
            csr([([1, 2, 3], [1.0, np.inf, 1.0])]),                               # a non-finite similarity
            csr([([1, 2, 3], [np.nan, 1.0, 1.0])]),
            csr([([1, 2, 3], one), ([9, 8, 9], one)]),                            # a neighbour twice in one list
        ]
        for off, nb, sm in bad:
            with pytest.raises(PgError) as e:
                p.dev.upload(off, nb, sm, 10)
            assert e.value.code == -1
            assert p.dev.info() == info
            assert_same(p.dev.cf_recall(trig, pref, 1500), before)
        with pytest.raises(PgError) as e:                                          # rows arrive in ascending order
            p.dev.upload(*csr([([1], [1.0])]), 4)
        assert e.value.code == -1
        assert_same(p.dev.cf_recall(trig, pref, 1500), before)
        p.upload([([1, 2, 3], one)], 11)                                           # ... and a good upload still lands (row 10 stays empty)
        assert p.dev.info()["pairs"] == info["pairs"] + 3
        p.check(trig, pref, 1500)
    finally:
        p.dev.destroy()


def test_generation_swap_makes_the_table_stale(ctx):
    t1, t2 = pa.Table(ctx, 300, DIM, 5), pa.Table(ctx, 300, DIM, 9)
    p = Pair(ctx, t1, 300, 5)
    try:
        p.upload([([1, 2, 3], [0.5, 0.25, 1.0]), ([3, 4], [1.0, 2.0])], 0)
        p.check([[0, 1]], [[1.0, 3.0]], 8)
        t1.swap(t2)
        with pytest.raises(PgError) as e:
            p.dev.cf_recall([[0, 1]], [[1.0, 3.0]], 8)
        assert e.value.code == -1 and "generation" in str(e.value)
    finally:
        p.dev.destroy()
        t1.destroy()
        t2.destroy()


# ---- exclusion ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
def test_exclusion_lists(base, normalize):
    rng = np.random.default_rng(51)
    trig = [rng.integers(0, ROWS, 25) for _ in range(5)]
    pref = [wide_prefer(rng, 25) for _ in range(5)]
    plain = ref.cf_recall(base.host, trig, pref, 5000, normalize)
    assert plain[2].min() > 400
    cand = [plain[0][q][:plain[2][q]] for q in range(5)]
    not_cand = np.setdiff1d(np.arange(ROW_OFFSET, ROW_OFFSET + ROWS, dtype=np.uint64), cand[2])
    lists = [
        np.zeros(0, np.uint64),                                                    # empty
        cand[1][:300].copy(),                                                      # the whole head
        np.concatenate([not_cand[:50], np.array([ref.U64MAX, 3, ROW_OFFSET + ROWS + 1], dtype=np.uint64)]),   # ids that are no candidates
        rng.choice(np.arange(ROW_OFFSET, ROW_OFFSET + ROWS, dtype=np.uint64), 4096, replace=False),  # 4 096 ids
        np.concatenate([cand[4][::2], cand[4][:7]]).astype(np.uint64)[:4096],      # every other candidate, some twice
    ]
    for k in (1, 200):
        got = base.check(trig, pref, k, normalize, lists)
        assert np.array_equal(got[0][0], plain[0][0][:k])
        assert got[0][1][0] == cand[1][300]
    base.check(trig, pref, 12000, normalize, lists)                                # deeper than any answer: padding behind the kept entries


def test_exclusion_depth_limit(base):
    lists = [np.arange(4096, dtype=np.uint64)]
    base.check([[70]], [[1.0]], 16384 - 4096, True, lists)
    with pytest.raises(PgError) as e:
        base.dev.cf_recall([[70]], [[1.0]], 16384 - 4095, True, lists)
    assert e.value.code == -4
    with pytest.raises(PgError) as e:
        base.dev.cf_recall([[70]], [[1.0]], 10, True, [np.arange(4097, dtype=np.uint64)])
    assert e.value.code == -4


# ---- device buffers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_lists", [False, True])
def test_dev_variant_equals_the_host_call(ctx, base, with_lists):
    rng = np.random.default_rng(61)
    trig = [rng.integers(0, ROWS, n) for n in (9, 0, 40)]
    pref = [wide_prefer(rng, len(t)) for t in trig]
    nq, k = 3, 333
    lists = [rng.choice(np.arange(ROW_OFFSET, ROW_OFFSET + ROWS, dtype=np.uint64), n, replace=False) for n in (100, 5, 900)] if with_lists else None
    want = base.dev.cf_recall(trig, pref, k, True, lists)
    off = np.zeros(nq + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in trig])
    bufs = [ctx.to_device(np.concatenate(trig).astype(np.uint32)), ctx.to_device(np.concatenate(pref).astype(np.float64)),
            ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 8)]
    try:
        d_excl, xoff = 0, None
        if with_lists:
            xoff = np.zeros(nq + 1, np.uint32)
            xoff[1:] = np.cumsum([len(l) for l in lists])
            bufs.append(ctx.to_device(np.concatenate(lists).astype(np.uint64)))
            d_excl = bufs[-1]
        counts = base.dev.cf_recall_dev(bufs[0], bufs[1], off, k, bufs[2], bufs[3], True, d_excl, xoff)
        rows, scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
        ctx.d2h(rows, bufs[2])
        ctx.d2h(scores, bufs[3])
    finally:
        for b in bufs:
            ctx.free(b)
    assert_same((rows, scores, counts), want)
