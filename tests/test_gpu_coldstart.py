"""GPU tests of ColdStartRecall (include/pairec_gpu.h "ColdStartRecall"; csrc/coldstart.hip): every answer by bits against
pg_cold_recall_host, which tests/test_coldstart_cpu.py holds against the independent restatement.

  grid          row counts around a bitmap word, a 1 024-row block and past many blocks; pools of no row, one row at either end, every
                row (no clause, and an always-true clause), every third row, only the last partial block, a dense block with a sparse
                rest; depths 1 .. 16 384 on both sides of the pool's size; 1, 3 and 256 requests; seeds 0, 1, 2^64 - 1, random, none
  ordered       I32 / I64 / F32 / F64 columns, ascending and descending: all values equal, two values whose tie runs straddle the k-th
                place and block boundaries, distinct values, the integer extremes, the floats' zeros, infinities, NaNs and subnormals;
                k = A and k = A + 1
  invalidation  a written clause column rebuilds bitmap and prefix once and changes the next answer, a written order column changes
                the answer and rebuilds nothing; a call enqueued before the write still answers for the old column
  chains        behind a stall, one stream, one synchronise: cold recall -> pg_exclude_compact_dev, and cold recall as one of three
                sources of pg_fanin_merge_dev
  refusals      on the host, the context usable and the next answer right"""
import ctypes as C

import numpy as np
import pytest

import coldstart_cases as cases
import coldstart_ref as ref
import fanin_ref
import pairec_amd as pa
from pairec_amd import _lib

pytestmark = pytest.mark.gpu

STALL_MS = 20
DIM = 64
DT_OF = {"i32": pa.F_I32, "i64": pa.F_I64, "f32": pa.F_F32, "f64": pa.F_F64}
FIXED_SEEDS = np.array([0, 1, (1 << 64) - 1], np.uint64)


class World:
    """one row count: the table, the store with the clause columns and the ordered columns, the compiled clauses, the host bitmaps"""

    def __init__(self, ctx, rows):
        self.ctx, self.rows = ctx, rows
        self.table = pa.Table(ctx, rows, DIM, row_offset=11)          # (its vectors are never read)
        self.fs = pa.Features(ctx, rows)
        self.masks, self.cols, self.ocols = cases.masks(rows), cases.store(rows), cases.order_columns(rows)
        for name, a in self.cols.items():
            self.fs.set_column(name, pa.F_I64 if a.dtype == np.int64 else pa.F_I32, a)
        for (dn, pattern), a in self.ocols.items():
            self.fs.set_column("%s_%s" % (dn, pattern), DT_OF[dn], a)
        self.where = {p: (pa.Where(c) if c is not None else None) for p, c in cases.POOLS.items()}
        self.bits = {p: (None if cases.POOLS[p] is None else cases.bitmap(self.masks[p])) for p in cases.POOLS}
        self.made = []

    def cold(self, pool, order_by=None):
        c = pa.ColdStart(self.where[pool], order_by)
        self.made.append(c)
        return c

    def close(self):
        for c in self.made:
            c.free()
        for w in self.where.values():
            if w is not None:
                w.free()
        self.fs.destroy()
        self.table.destroy()


@pytest.fixture(scope="module")
def worlds(ctx):
    made = {}

    def get(rows):
        if rows not in made:
            made[rows] = World(ctx, rows)
        return made[rows]
    yield get
    for w in made.values():
        w.close()


def _seeds(rng, nq, kind):
    if kind == "none":
        return None
    if kind == "fixed":
        return np.resize(FIXED_SEEDS, nq)
    return rng.integers(0, 1 << 63, nq).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, nq).astype(np.uint64)


@pytest.mark.parametrize("rows", cases.ROWS)
def test_random_order_grid(ctx, worlds, rows):
    w = worlds(rows)
    rng = np.random.default_rng(rows)
    nq_of = {1: 256, 7: 3, 256: 256, 257: 1, 4096: 3, 16384: 1}
    for pool in cases.POOLS:
        c = w.cold(pool)
        for k in cases.KS:
            for kind in (("fixed", "none") if k in (1, 257, 4096) else ("random", "fixed")):
                nq = nq_of[k]
                sd = _seeds(rng, nq, kind)
                got = c.recall(ctx, w.table, w.fs if pool != "all_null" or k == 7 else None, nq, k, seed=sd)
                want = c.recall_host(rows, nq, k, bits=w.bits[pool], seed=sd, row_offset=11)
                ref.same(got, want, "rows %d pool %s k %d nq %d seeds %s" % (rows, pool, k, nq, kind))
        st = c.stats()
        assert st["prefix_builds"] == 1 and st["admitted"] == int(w.masks[pool].sum()), (pool, st)


def test_random_order_full_shape(ctx, worlds):
    """256 requests at depth 16 384 — the largest output — over a pool smaller and a pool larger than the depth"""
    w = worlds(40000)
    sd = _seeds(np.random.default_rng(5), 256, "random")
    for pool in ("third", "all_true"):
        c = w.cold(pool)
        ref.same(c.recall(ctx, w.table, w.fs, 256, 16384, seed=sd), c.recall_host(40000, 256, 16384, bits=w.bits[pool], seed=sd, row_offset=11), pool)


@pytest.mark.parametrize("rows", (1, 33, 1025, 40000, 300001))
def test_ordered_grid(ctx, worlds, rows):
    w = worlds(rows)
    pools = ("third",) if rows > 40000 else ("all_null", "third", "dense_sparse", "none", "last")
    for (dn, pattern), col in w.ocols.items():
        for direction in ("ASC", "desc"):
            for pool in pools:
                c = w.cold(pool, "%s_%s %s" % (dn, pattern, direction))
                A = int(w.masks[pool].sum())
                ks = (7, 4096, 16384) if rows > 40000 else sorted({1, 256, 4096, 16384, min(max(A, 1), 16384), min(A + 1, 16384)})
                for k in ks:
                    nq = 3 if k < 4096 else 1
                    got = c.recall(ctx, w.table, w.fs, nq, k, seed=FIXED_SEEDS[:nq])          # (seeds are ignored)
                    want = c.recall_host(rows, nq, k, bits=w.bits[pool], order_col=col, row_offset=11)
                    ref.same(got, want, "rows %d %s %s %s pool %s k %d" % (rows, dn, pattern, direction, pool, k))


@pytest.mark.parametrize("k", (511, 512, 513, 1024, 1025, 8191, 8192, 8193))
def test_ordered_at_the_final_sorts_sizes(ctx, worlds, k):
    """around one run of the split sort, two runs, and its largest list — above which the survivors are ordered by counting"""
    w = worlds(40000)
    for pool, column, key in (("all_true", "i32_two", ("i32", "two")), ("third", "f32_special desc", ("f32", "special")),
                              ("all_null", "i64_equal desc", ("i64", "equal"))):
        c = w.cold(pool, column)
        ref.same(c.recall(ctx, w.table, w.fs, 2, k), c.recall_host(40000, 2, k, bits=w.bits[pool], order_col=w.ocols[key], row_offset=11),
                 "%s %s k %d" % (pool, column, k))


def test_ordered_256_requests(ctx, worlds):
    w = worlds(40000)
    c = w.cold("third", "f64_special desc")
    ref.same(c.recall(ctx, w.table, w.fs, 256, 257), c.recall_host(40000, 256, 257, bits=w.bits["third"], order_col=w.ocols["f64", "special"], row_offset=11))


class Bufs:
    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def put(self, a):
        self.all.append(self.ctx.to_device(a))
        return self.all[-1]

    def new(self, nbytes):
        self.all.append(self.ctx.malloc(max(nbytes, 16)))
        return self.all[-1]

    def get(self, p, shape, dtype):
        a = np.empty(shape, dtype)
        self.ctx.d2h(a, p)
        return a

    def free(self):
        for p in self.all:
            self.ctx.free(p)


def test_column_writes_invalidate(ctx):
    rows, nq, k = 5000, 4, 300
    rng = np.random.default_rng(9)
    status = (rng.random(rows) < 0.3).astype(np.int32)
    stock = rng.integers(0, 5, rows).astype(np.int64)
    ct = rng.integers(0, 1000, rows).astype(np.int64)
    table, fs = pa.Table(ctx, rows, DIM), pa.Features(ctx, rows)
    fs.set_column("status", pa.F_I32, status)
    fs.set_column("stock", pa.F_I64, stock)
    fs.set_column("create_time", pa.F_I64, ct)
    w = pa.Where("status = 1 AND stock > 0")
    rnd, top = pa.ColdStart(w, None), pa.ColdStart(w, "create_time DESC")
    sd = np.array([5, 6, 7, 8], np.uint64)
    b = Bufs(ctx)
    try:
        bits0 = w.eval_host({"status": status, "stock": stock})
        ref.same(rnd.recall(ctx, table, fs, nq, k, seed=sd), rnd.recall_host(rows, nq, k, bits=bits0, seed=sd), "first")
        ref.same(rnd.recall(ctx, table, fs, nq, k, seed=sd), rnd.recall_host(rows, nq, k, bits=bits0, seed=sd), "again")
        ref.same(top.recall(ctx, table, fs, nq, k), top.recall_host(rows, nq, k, bits=bits0, order_col=ct), "top first")
        assert (rnd.stats()["prefix_builds"], rnd.stats()["prefix_hits"], top.stats()["prefix_builds"], w.stats()["builds"]) == (1, 1, 1, 1)
        # a call enqueued before the write answers for the old column: the write is ordered behind it on the stream
        d_seed, d_r0, d_s0, d_c0 = b.put(sd), b.new(nq * k * 8), b.new(nq * k * 4), b.new(nq * 4)
        ctx.debug_stall(STALL_MS)
        rnd.recall_dev(ctx, table, fs, d_seed, nq, k, d_r0, d_s0, d_c0)
        status2 = 1 - status
        fs.set_column("status", pa.F_I32, status2)
        bits1 = w.eval_host({"status": status2, "stock": stock})
        new = rnd.recall(ctx, table, fs, nq, k, seed=sd)
        old = (b.get(d_r0, (nq, k), np.uint64), b.get(d_s0, (nq, k), np.float32), b.get(d_c0, nq, np.uint32))
        ref.same(old, rnd.recall_host(rows, nq, k, bits=bits0, seed=sd), "enqueued before the write")
        ref.same(new, rnd.recall_host(rows, nq, k, bits=bits1, seed=sd), "after the write")
        assert not np.array_equal(old[0], new[0])
        assert (rnd.stats()["prefix_builds"], w.stats()["builds"]) == (2, 2)           # one rebuild each
        ref.same(top.recall(ctx, table, fs, nq, k), top.recall_host(rows, nq, k, bits=bits1, order_col=ct), "top after the clause write")
        assert (top.stats()["prefix_builds"], w.stats()["builds"]) == (2, 2)           # (the bitmap is shared: built once for both)
        # the order column: the next answer changes, nothing is rebuilt
        before = top.recall(ctx, table, fs, nq, k)
        ct2 = ct[::-1].copy()
        fs.set_column("create_time", pa.F_I64, ct2)
        after = top.recall(ctx, table, fs, nq, k)
        ref.same(after, top.recall_host(rows, nq, k, bits=bits1, order_col=ct2), "after the order column's write")
        assert not np.array_equal(before[0], after[0])
        assert (top.stats()["prefix_builds"], w.stats()["builds"]) == (2, 2)
    finally:
        b.free()
        rnd.free()
        top.free()
        w.free()
        fs.destroy()
        table.destroy()


def test_chains_behind_a_stall(ctx, worlds):
    """cold recall at depth k + L -> pg_exclude_compact_dev, and a random and an ordered cold recall as two of three sources of
    pg_fanin_merge_dev: every enqueue precedes the device's first kernel, one synchronise at the end"""
    w = worlds(40000)
    rows, nq, k, L = 40000, 5, 50, 9
    rng = np.random.default_rng(77)
    c = w.cold("dense_sparse")
    top = w.cold("third", "i64_two desc")
    sd = _seeds(rng, nq, "random")
    deep = c.recall_host(rows, nq, k + L, bits=w.bits["dense_sparse"], seed=sd, row_offset=11)
    head = top.recall_host(rows, nq, 40, bits=w.bits["third"], order_col=w.ocols["i64", "two"], row_offset=11)
    # each request excludes L ids: some from the head of its own sequence, some it will never see
    lists = [np.concatenate([deep[0][q, rng.choice(k, L - 3, replace=False)], np.array([5, (1 << 64) - 1, deep[0][q, 0]], np.uint64)]) for q in range(nq)]
    want_ex = np.full((nq, k), (1 << 64) - 1, np.uint64)
    for q in range(nq):
        keep = [r for r in deep[0][q].tolist() if r not in set(lists[q].tolist())][:k]
        want_ex[q, :len(keep)] = keep
    src1 = (np.concatenate([head[0][:, 5:25], rng.integers(0, rows, (nq, 10)).astype(np.uint64) + np.uint64(11)], axis=1), rng.random((nq, 30)))
    src1[0][:, :4] = deep[0][:, :4]                                  # duplicates across recalls
    want_fan = fanin_ref.merge([src1, (deep[0][:, :k].copy(), deep[1][:, :k].copy()), head[:2]])
    c.recall(ctx, w.table, w.fs, nq, k + L, seed=sd)                 # bitmaps, prefixes and scratch exist before the stall
    top.recall(ctx, w.table, w.fs, nq, 40)
    b = Bufs(ctx)
    try:
        d_seed = b.put(sd)
        d_ids, d_off = b.put(np.concatenate(lists)), b.put(np.arange(nq + 1, dtype=np.uint32) * np.uint32(L))
        d_deep_r, d_deep_s = b.new(nq * (k + L) * 8), b.new(nq * (k + L) * 4)
        d_ex_r, d_ex_s, d_ex_c = b.new(nq * k * 8), b.new(nq * k * 4), b.new(nq * 4)
        d_cold_r, d_cold_s, d_cold_c = b.new(nq * k * 8), b.new(nq * k * 4), b.new(nq * 4)
        d_top_r, d_top_s = b.new(nq * 40 * 8), b.new(nq * 40 * 4)
        d_src1 = (b.put(src1[0]), b.put(src1[1]))
        cap = 30 + k + 40
        d_out = [b.new(nq * cap * 8), b.new(nq * cap * 8), b.new(nq * cap), b.new(3 * nq * cap * 8), b.new(nq * cap * 4), b.new(nq * 4)]
        hits = c.stats()["prefix_hits"]
        ctx.debug_stall(STALL_MS)
        c.recall_dev(ctx, w.table, w.fs, d_seed, nq, k + L, d_deep_r, d_deep_s)
        _lib.check(ctx.L.pg_exclude_compact_dev(ctx.h, C.c_void_p(d_deep_r), C.c_void_p(d_deep_s), nq, k + L, C.c_void_p(d_ids), C.c_void_p(d_off), k,
                                                float("-inf"), C.c_void_p(d_ex_r), C.c_void_p(d_ex_s), C.c_void_p(d_ex_c)))
        c.recall_dev(ctx, w.table, w.fs, d_seed, nq, k, d_cold_r, d_cold_s, d_cold_c)
        top.recall_dev(ctx, w.table, w.fs, 0, nq, 40, d_top_r, d_top_s)
        ctx.fanin_merge_dev([(d_src1[0], d_src1[1], 30, True), (d_cold_r, d_cold_s, k, False), (d_top_r, d_top_s, 40, False)], nq, *d_out)
        ctx.synchronize()
        assert c.stats()["prefix_hits"] == hits + 2 and c.stats()["prefix_builds"] == 1
        ex_r, ex_c = b.get(d_ex_r, (nq, k), np.uint64), b.get(d_ex_c, nq, np.uint32)
        assert np.array_equal(ex_r, want_ex) and np.array_equal(ex_c, (want_ex != np.uint64((1 << 64) - 1)).sum(axis=1))
        assert np.array_equal(b.get(d_ex_s, (nq, k), np.float32).view(np.uint32), np.where(want_ex != np.uint64((1 << 64) - 1), np.float32(0), np.float32(-np.inf)).astype(np.float32).view(np.uint32))
        assert np.array_equal(b.get(d_cold_c, nq, np.uint32), np.full(nq, k, np.uint32))
        got = (b.get(d_out[0], (nq, cap), np.uint64), b.get(d_out[1], (nq, cap), np.float64), b.get(d_out[2], (nq, cap), np.uint8),
               b.get(d_out[3], (3, nq, cap), np.float64), b.get(d_out[4], (nq, cap), np.uint32), b.get(d_out[5], nq, np.uint32))
        fanin_ref.same(got, want_fan)
    finally:
        b.free()


def test_refusals_leave_the_context_usable(ctx, worlds):
    w = worlds(1025)
    c = w.cold("third")
    short = pa.Features(ctx, 1000)
    short.set_column("m_third", pa.F_I32, cases.store(1000)["m_third"])
    short.set_column("one", pa.F_I64, np.ones(1000, np.int64))
    w.fs.set_column("declared", pa.F_I32, None, default=4)
    w.fs.set_column("text", pa.F_F32, np.zeros(1025, np.float32))
    try:
        for args, code in (((w.fs, 1, 0), -4), ((w.fs, 1, 16385), -4), ((w.fs, 257, 1), -1), ((w.fs, 0, 1), -1), ((short, 1, 5), -1), ((None, 1, 5), -1)):
            with pytest.raises(_lib.PgError) as e:
                c.recall(ctx, w.table, args[0], args[1], args[2])
            assert e.value.code == code, (args[1:], str(e.value))
            ref.same(c.recall(ctx, w.table, w.fs, 2, 9, seed=[1, 2]), c.recall_host(1025, 2, 9, bits=w.bits["third"], seed=[1, 2], row_offset=11), "after a refusal")
        unknown = w.cold("third", "nope desc")
        with pytest.raises(_lib.PgError) as e:
            unknown.recall(ctx, w.table, w.fs, 1, 5)
        assert e.value.code == -1 and "nope" in str(e.value)
        bad_clause = pa.ColdStart(pa.Where("text > 0"), None)            # a clause over a float column: pg_where's Binding rule
        with pytest.raises(_lib.PgError) as e:
            bad_clause.recall(ctx, w.table, w.fs, 1, 5)
        assert e.value.code == -1
        bad_clause.where.free()
        bad_clause.free()
        # a column declared without values holds its default in every row: it is an ordered column of equal values
        declared = w.cold("third", "declared desc")
        ref.same(declared.recall(ctx, w.table, w.fs, 1, 5), declared.recall_host(1025, 1, 5, bits=w.bits["third"], order_col=np.full(1025, 4, np.int32), row_offset=11))
        ref.same(c.recall(ctx, w.table, w.fs, 2, 9, seed=[1, 2]), c.recall_host(1025, 2, 9, bits=w.bits["third"], seed=[1, 2], row_offset=11), "at the end")
    finally:
        short.destroy()
