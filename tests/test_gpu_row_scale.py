"""GPU tests of row selection past one scan group of rows.  Three components choose rows of a table by a predicate, all three in
1 024-row blocks whose counts are scanned in a second and a third level, and every other test of them stays inside the first group
of blocks and the first trip of a grid-stride loop:

    code                                              first level       second level, from                  third level / second trip, from
    recall_filter.hip  filter_block_count_kernel,     1 024 rows        1 024 blocks a group:               filter_total_scan_kernel's thread 1
                       filter_group_scan_kernel,      a block           group_off[blockIdx.x >> 10] above   holds groups 4..7:
                       filter_total_scan_kernel,                        index 0 from 1 048 577 rows         4 194 305 rows
                       filter_scatter_kernel (views,
                       the compact path of
                       pg_recall_topk_where[_ex])
    where.hip          where_eval_kernel (the bitmap  1 024-row tiles   grid = min(tiles, 8 x CUs): a       -
                       of a compound clause)                            second trip of the tile loop (LDS
                                                                        term words reused, the count kept
                                                                        across trips) from 2 097 153 rows
    coldstart.hip      scan_launch (sums / top /      1 024-row blocks  kScanChunk = 1 024 blocks:          cold_hist_kernel's second trip
                       apply), cold_sample_kernel's                     sums[blockIdx.x] above block 0      from 2 097 153 rows
                       search in the prefix,                            from 1 048 577 rows
                       cold_hist_kernel (grid-stride),
                       cold_tile_count_kernel +
                       cold_collect_kernel (scan[blockIdx.x])

(row counts for 256 CUs; the grid comes from the device).  The table here has row_scale_cases.rows_for(CUs) rows, 4 199 427 at 256
CUs: five groups and chunks, the fifth partial; two full trips and a ragged last; a last block of 3 rows.  tests/row_scale_cases.py
builds the masks, each to stress one place, the store that states every mask as an int32 flag, an int64 flag and a compound
clause, and a table whose rows name themselves; tests/test_row_scale_cpu.py shows that the cases meet these conditions and holds
the two host mirrors used below to numpy.  Everything is compared by bits or as integers: no tolerance anywhere.

  a  every clause's device bitmap == np.packbits of the numpy mask == pg_where_eval_host, the count == mask.sum(); again at
     rows - 3 (a multiple of 1 024) and at 8 x CUs x 1 024 + 1 rows (one row into the second trip)
  b  the compaction seen directly: views by int32 flag, int64 flag and clause hold exactly the rows np.nonzero(mask) names, in
     order, every column bit for bit; the failure names the first wrong position, its block and its group
  c  recalls on top (inner product and squared Euclidean, 1 and 40 queries, k = 300) over the view, through
     pg_recall_topk_where[_ex] at the default "where_compact_max_rows" and in place, against the oracle on tab[idx]; two pairs of
     duplicate rows, one across the first group boundary of the table and one across it in the `eighth` view, lead query 0's
     inner-product answer, so the tie order across a group's first offset is observed.  (Under squared Euclidean the two index
     columns enter the distance: the pairs do not tie there.)  `one_group` is a quarter of the rows, so the product serves it
     in place like `eighth`; `last_group`, beyond the issue's three masks, is the one-group mask the compact path takes
  d  ColdStart pools: random order against pg_cold_recall_host and, independently, distinct admitted rows and counts; ordered by
     two values whose runs cross the chunk boundaries, by a permutation, by the floats' special values

filter_total_scan_kernel beyond its first wave would need more than 256 groups, 268 M rows: no test-sized table reaches that.  The
cross-wave part of block_excl_scan<16> is exercised by filter_group_scan_kernel in every case here."""
import time

import numpy as np
import pytest

import coldstart_ref as ref
import pairec_amd as pa
import row_scale_cases as cases
from oracle import oracle as o
from pairec_amd import _lib
from row_scale_cases import BLOCK, G, ROW_OFFSET

pytestmark = pytest.mark.gpu

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
COMPACT_DEFAULT = 8 << 20        # "where_compact_max_rows" default
K = cases.K_RECALL
SEL = (0, 20, 39)                # the queries of a 40-query call that are held to the oracle
FIXED_SEEDS = np.array([0, 1, (1 << 64) - 1], np.uint64)
ORDERS = (("i32_two ASC", "i32_two"), ("i32_two desc", "i32_two"), ("i64_distinct", "i64_distinct"), ("f32_special desc", "f32_special"))
POOLS = ("edges", "sparse", "eighth", "trip_tail", "all", "none")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


class World:
    def __init__(self, ctx):
        self.cus = cases.device_cus()
        self.rows = rows = cases.rows_for(self.cus)
        self.masks, self.cols, self.clauses = cases.masks(rows, self.cus), cases.store(rows, self.cus), cases.clauses(rows, self.cus)
        self.ocols = cases.order_columns(rows)
        self.tab = cases.table(rows, self.masks["eighth"])
        self.pairs = cases.dup_pairs(self.masks["eighth"])
        self.q = cases.queries()
        self.t = pa.Table(ctx, rows, cases.DIM, row_offset=ROW_OFFSET)
        self.t.upload(self.tab)
        self.feats = pa.Features(ctx, rows)
        for name, a in {**self.cols, **self.ocols}.items():
            self.feats.set_column(name, {np.int32: pa.F_I32, np.int64: pa.F_I64, np.float32: pa.F_F32}[a.dtype.type], a)
        self._idx, self._sub, self._oracle = {}, {}, {}

    def idx(self, name):
        if name not in self._idx:
            self._idx[name] = np.flatnonzero(self.masks[name])
        return self._idx[name]

    def sub(self, name):
        """tab[idx]: the admitted rows, shared by the tests of one mask and never changed"""
        if name not in self._sub:
            self._sub.clear()                                  # (one at a time: `eighth`'s is 139 MB)
            self._sub[name] = self.tab[self.idx(name)]
        return self._sub[name]

    def oracle(self, name, l2):
        """the oracle on the admitted rows for the queries SEL, mapped back through idx + ROW_OFFSET"""
        if (name, l2) not in self._oracle:
            idx = self.idx(name)
            orow, osc = (o.recall_topk_l2 if l2 else o.recall_topk)(self.sub(name), self.q[list(SEL)], K)
            assert orow.shape == (len(SEL), min(K, idx.size))
            self._oracle[name, l2] = ((idx[orow.astype(np.int64)] + ROW_OFFSET).astype(np.uint64), osc)
        return self._oracle[name, l2]

    def close(self):
        self.feats.destroy()
        self.t.destroy()


@pytest.fixture(scope="module")
def world(ctx):
    t0 = time.perf_counter()
    w = World(ctx)
    print("\nrow scale: %d CUs -> %d rows, %s; world built in %.1f s" % (w.cus, w.rows, cases.shape(w.rows, w.cus), time.perf_counter() - t0))
    yield w
    w.close()


def test_the_device_meets_the_cases_conditions(world):
    s = cases.shape(world.rows, world.cus)
    assert s["groups"] == 5 and s["blocks"] % 1024 and s["blocks"] > 2 * s["grid"] and s["blocks"] % s["grid"] and s["last_block_rows"] == 3
    assert world.cus < 256 or s["trips"] == 3


# ---- a. the bitmap ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", ["rows", "rows - 3", "one row into the second trip"])
def test_bitmap(ctx, world, at):
    n = {"rows": world.rows, "rows - 3": world.rows - 3, "one row into the second trip": 8 * world.cus * BLOCK + 1}[at]
    assert n <= world.rows and (at != "rows - 3" or n % BLOCK == 0)
    for name, (clause, in_numpy) in world.clauses.items():
        mask = in_numpy(world.cols)[:n]
        want = np.packbits(mask, bitorder="little")
        want = np.concatenate([want, np.zeros(-want.size % 4, np.uint8)]).view("<u4")
        w = pa.Where(clause)
        try:
            dev, admitted = w.bits(ctx, world.feats, n)
            host = w.eval_host({c: world.cols[c][:n] for c in w.columns}, n)
            assert w.stats()["builds"] == 1
        finally:
            w.free()
        if not np.array_equal(dev, want):
            word = int(np.flatnonzero(dev != want)[0])
            raise AssertionError("%s at %d rows: bitmap word %d (tile %d, trip %d) is %#x, numpy has %#x; %d words differ" %
                                 (name, n, word, word // 32, word // 32 // (8 * world.cus), dev[word], want[word], int((dev != want).sum())))
        assert admitted == int(mask.sum()), (name, n, admitted, int(mask.sum()))
        assert np.array_equal(dev, host), (name, n)


# ---- b. the compaction, seen directly -----------------------------------------------------------------------------------------------
def view_kinds(world, name):
    t, f = world.t, world.feats
    yield "int32 flag", lambda: t.view(f, "f_" + name, "==", 1), None
    yield "int64 flag", lambda: t.view(f, "g_" + name, ">", cases.BIG), None
    w = pa.Where(world.clauses[name][0])
    yield "clause", lambda: t.view_where(f, w), w


@pytest.mark.parametrize("name", cases.VIEW_MASKS)
def test_view_holds_the_admitted_rows_in_order(ctx, world, name):
    idx = world.idx(name)
    for kind, make, w in view_kinds(world, name):
        try:
            v = make()
        finally:
            if w is not None:
                w.free()
        try:
            assert v.rows == idx.size, (name, kind, v.rows, idx.size)
            got = v.download(0, v.rows)
        finally:
            v.destroy()
        src = cases.decode(got)
        if not np.array_equal(src, idx):
            p = int(np.flatnonzero(src != idx)[0])
            raise AssertionError("%s view by %s: position %d holds row %d, not row %d (block %d, group %d; %d of %d positions differ)" %
                                 (name, kind, p, src[p], idx[p], idx[p] // BLOCK, idx[p] // G, int((src != idx).sum()), idx.size))
        assert np.array_equal(bits(got), bits(world.sub(name))), (name, kind)


def test_view_of_no_row_is_refused(ctx, world):
    for kind, make, w in view_kinds(world, "none"):
        with pytest.raises(_lib.PgError) as e:
            make()
        if w is not None:
            w.free()
        assert e.value.code == -8, (kind, str(e.value))                      # PG_ERR_EMPTY


# ---- c. recalls on top ----------------------------------------------------------------------------------------------------------------
def check_vs_oracle(world, got, name, l2, nq, what):
    m = min(K, world.idx(name).size)
    assert got[2].tolist() == [m] * nq, (what, got[2][:4])
    assert np.all(got[0][:, m:] == U64MAX), what
    orow, osc = world.oracle(name, l2)
    sel = [0] if nq == 1 else list(SEL)
    for i, qi in enumerate(sel):
        if not np.array_equal(got[0][qi, :m], orow[i]):
            p = int(np.flatnonzero(got[0][qi, :m] != orow[i])[0])
            raise AssertionError("%s, query %d: place %d holds row %d, the oracle row %d (block %d, group %d)" %
                                 (what, qi, p, int(got[0][qi, p]) - ROW_OFFSET, int(orow[i][p]) - ROW_OFFSET,
                                  (int(orow[i][p]) - ROW_OFFSET) // BLOCK, (int(orow[i][p]) - ROW_OFFSET) // G))
        assert np.array_equal(bits(got[1][qi, :m]), bits(osc[i])), (what, qi)


@pytest.mark.parametrize("l2", [False, True], ids=["ip", "l2"])
@pytest.mark.parametrize("name", ["edges", "one_group", "eighth", "last_group"])
def test_recalls_over_the_admitted_rows(ctx, world, name, l2):
    t, f, mask = world.t, world.feats, world.masks[name]
    orow, osc = world.oracle(name, l2)
    if not l2:
        # the duplicate pairs the mask admits lead query 0's answer, each pair tied and in row order: the tie order is tested
        admitted = [p for p in world.pairs if mask[list(p)].all()]
        assert len(admitted) >= {"edges": 2, "eighth": 1}.get(name, 0)
        for a, b in admitted:
            at = np.flatnonzero(orow[0] == a + ROW_OFFSET)
            assert at.size == 1 and at[0] < 5 and orow[0][at[0] + 1] == b + ROW_OFFSET and bits(osc[0])[at[0]] == bits(osc[0])[at[0] + 1], (name, a, b)
    w = pa.Where(world.clauses[name][0])
    v_flag, v_where = t.view(f, "f_" + name, "==", 1), t.view_where(f, w)
    try:
        for nq in (1, 40):
            q = world.q[:nq]
            for kind, v in (("flag", v_flag), ("clause", v_where)):
                check_vs_oracle(world, (v.recall_topk_l2 if l2 else v.recall_topk)(q, K), name, l2, nq, "%s view by %s, nq %d" % (name, kind, nq))
            for compact_max in (COMPACT_DEFAULT, 0):
                try:
                    ctx.set_option("where_compact_max_rows", compact_max)
                    what = "%s nq %d where_compact_max_rows %d" % (name, nq, compact_max)
                    check_vs_oracle(world, t.recall_topk_where(f, "f_" + name, "==", 1, q, K, l2=l2), name, l2, nq, what + " int32 flag")
                    check_vs_oracle(world, t.recall_topk_where(f, "g_" + name, "!=", cases.BIG, q, K, l2=l2), name, l2, nq, what + " int64 flag")
                    check_vs_oracle(world, t.recall_topk_where_ex(f, w, q, K, l2=l2), name, l2, nq, what + " clause")
                finally:
                    ctx.set_option("where_compact_max_rows", COMPACT_DEFAULT)
        assert w.stats()["admitted"] == int(mask.sum())
    finally:
        v_flag.destroy()
        v_where.destroy()
        w.free()


# ---- d. ColdStart pools -----------------------------------------------------------------------------------------------------------------
def pool_of(world, pool):
    """(the clause or None, the host bitmap or None, the admitted rows)"""
    if pool == "all":
        return None, None, world.idx("all")
    return pa.Where(world.clauses[pool][0]), cases.bitmap(world.masks[pool]), world.idx(pool)


@pytest.mark.parametrize("pool", POOLS)
def test_cold_random_order(ctx, world, pool):
    w, bm, idx = pool_of(world, pool)
    A = idx.size
    rng = np.random.default_rng(A + 1)
    c = pa.ColdStart(w, None)
    try:
        for k in (7, 4096, 16384):
            for sd in (FIXED_SEEDS, rng.integers(0, 1 << 63, 3).astype(np.uint64) * np.uint64(2) + np.uint64(1)):
                got = c.recall(ctx, world.t, world.feats, 3, k, seed=sd)
                ref.same(got, c.recall_host(world.rows, 3, k, bits=bm, seed=sd, row_offset=ROW_OFFSET), "pool %s k %d seeds %s" % (pool, k, sd))
                kk = min(k, A)                                               # ... and without the mirror
                assert got[2].tolist() == [kk] * 3 and np.all(got[0][:, kk:] == U64MAX)
                for r in range(3):
                    rows = got[0][r, :kk].astype(np.int64) - ROW_OFFSET
                    assert np.unique(rows).size == kk and rows.min(initial=0) >= 0 and rows.max(initial=0) < world.rows
                    assert world.masks[pool][rows].all(), (pool, k, r)
        st = c.stats()
        assert st["prefix_builds"] == 1 and st["admitted"] == A, (pool, st)
    finally:
        c.free()
        if w is not None:
            w.free()


@pytest.mark.parametrize("pool", POOLS)
def test_cold_ordered(ctx, world, pool):
    w, bm, idx = pool_of(world, pool)
    try:
        for order_by, col in ORDERS:
            c = pa.ColdStart(w, order_by)
            try:
                for k in (7, 4096, 16384):
                    got = c.recall(ctx, world.t, world.feats, 1, k)
                    want = c.recall_host(world.rows, 1, k, bits=bm, order_col=world.ocols[col], row_offset=ROW_OFFSET)
                    ref.same(got, want, "pool %s %s k %d" % (pool, order_by, k))
                st = c.stats()
                assert st["prefix_builds"] == 1 and st["admitted"] == idx.size, (pool, order_by, st)
            finally:
                c.free()
    finally:
        if w is not None:
            w.free()
