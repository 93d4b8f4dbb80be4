"""GPU tests of the list recall on the device (csrc/hot.hip: pg_hottable_*, pg_hot_recall_dev, pg_hot_recall)
against tests/hot_ref.py: rows, counts and sources as integers, scores as bit patterns.  The table and the grid are
tests/hot_cases.py's (the CPU test runs pg_hot_recall_host over the same cases): one hot table over an item table of 70 000 x 64
rows whose global ids end just below 2^32 (row_offset 4 000 000 000).  Every output buffer of a device call carries a guard region behind it, pre-filled."""
import re

import numpy as np
import pytest

import fanin_ref
import hot_cases as cases
import hot_ref as ref
import pairec_amd as pa
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID, UNSUPPORTED = -1, -4


class Guarded:
    """device buffers with a guard behind every one: outputs are pre-filled, so an element the kernel skips shows as well"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a):
        if a is None:
            return 0
        p = self.ctx.to_device(np.ascontiguousarray(a))
        self.bufs.append((p, None, 0))
        return p

    def out(self, a):
        if a is None:
            return 0
        p = self.ctx.malloc(a.nbytes + GUARD)
        self.ctx.h2d(p, np.full(a.nbytes + GUARD, 0xA5, np.uint8))
        self.bufs.append((p, a, a.nbytes))
        return p

    def fetch(self):
        self.ctx.synchronize()
        for p, a, nbytes in self.bufs:
            if a is None:
                continue
            raw = np.empty(nbytes + GUARD, np.uint8)
            self.ctx.d2h(raw, p)
            assert np.all(raw[nbytes:] == 0xA5), "a write behind an output"
            a.reshape(-1).view(np.uint8)[:] = raw[:nbytes]

    def untouched(self):
        """every output still holds its pre-fill, guard included"""
        self.ctx.synchronize()
        for p, a, nbytes in self.bufs:
            if a is not None:
                raw = np.empty(nbytes + GUARD, np.uint8)
                self.ctx.d2h(raw, p)
                assert np.all(raw == 0xA5), "a refused call wrote an output"

    def free(self):
        for p, _, _ in self.bufs:
            self.ctx.free(p)


def outs_of(nq, k, source=True, count=True):
    return [np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64), np.empty((nq, k), np.uint8) if source else None,
            np.empty(nq, np.uint32) if count else None]


def recall_dev(ctx, g, hot, mode, trig, k, values=None, seed=None, source=True, count=True):
    """one pg_hot_recall_dev launch → its (unfetched) outputs"""
    outs = outs_of(len(trig), k, source, count)
    d = [g.out(a) for a in outs]
    ctx.hot_recall_dev(hot, mode, trig, k, d[0], d[1], d[2], d[3], values=values, d_seed=g.put(None if seed is None else np.asarray(seed, np.uint64)))
    return outs, d


@pytest.fixture(scope="module")
def base(ctx):
    t = pa.Table(ctx, cases.ROWS, cases.DIM, cases.ROW_OFFSET)
    hot = ctx.hottable_create(t, cases.N_TRIGGERS)
    fresh = ctx.hottable_info(hot)
    assert fresh == {"rows": cases.ROWS, "n_triggers": cases.N_TRIGGERS, "pairs": 0, "triggers_uploaded": 0, "generation": fresh["generation"]}
    # a recall before any upload: every list is empty
    got = ctx.hot_recall(hot, ref.GROUP, [[0, 1, cases.T_MAX], []], 7)
    assert not got[3].any() and np.all(got[0] == ref.PAD_ROW) and np.all(np.isneginf(got[1])) and np.all(got[2] == 0xFF)
    uploads, whole = cases.table()
    for trig0, off, rows, sc, src in uploads:
        hot.upload(off, rows, sc, src, trig0)
    assert ctx.hottable_info(hot) == dict(fresh, pairs=len(whole[1]), triggers_uploaded=cases.T_LATE + 1)
    yield t, hot
    hot.destroy()
    t.destroy()


@pytest.mark.parametrize("name", sorted(cases.grid()))
def test_grid(ctx, base, name):
    _, hot = base
    mode, trig, values, seed, k = cases.grid()[name]
    want = cases.expected(name)
    g = Guarded(ctx)
    try:
        outs, _ = recall_dev(ctx, g, hot, mode, trig, k, values, seed)
        bare, _ = recall_dev(ctx, g, hot, mode, trig, k, values, seed, source=False, count=False)     # the optional outputs left out
        g.fetch()
        ref.same(outs, want)
        ref.same(bare[:2] + [None, want[3]], want)
    finally:
        g.free()
    if "batch" not in name and "max_entries" not in name:
        ref.same(ctx.hot_recall(hot, mode, trig, k, values, seed), want)                           # the host-array entry is the same call


def test_batching_invariance(ctx, base):
    """a request answers the same alone as in its batch of 256 (its tier and its slice of the scratch are its own)"""
    _, hot = base
    mode, trig, values, seed, k = cases.grid()["global_batch_256"]
    want = cases.expected("global_batch_256")
    for q in (0, 3, 6, 7, 255):
        ref.same(ctx.hot_recall(hot, mode, [trig[q]], k, None, [seed[q]]), tuple(w[q:q + 1] for w in want))


def test_refusals_enqueue_nothing_and_leave_the_context_usable(ctx, base):
    _, hot = base
    g = Guarded(ctx)
    try:
        for trig, q in cases.TOO_LONG:
            with pytest.raises(PgError) as e:
                recall_dev(ctx, g, hot, ref.GROUP, trig, 16)
            assert e.value.code == UNSUPPORTED and "request %d concatenates 65537 entries" % q in str(e.value)
        for args, code, what in ((dict(mode=3, trig=[[1]], k=4), INVALID, "mode 3"), (dict(mode=0, trig=[[1]], k=16385), UNSUPPORTED, "k=16385"),
                                 (dict(mode=0, trig=[[1]] * 257, k=4), INVALID, "nq=257"),
                                 (dict(mode=0, trig=[[1] * 257], k=4), UNSUPPORTED, "257 triggers"),
                                 (dict(mode=2, trig=[[1], [2, 3]], k=4, values=[[1.0], [1.0, np.nan]]), INVALID, "trigger 1 of request 1")):
            with pytest.raises(PgError) as e:
                recall_dev(ctx, g, hot, args["mode"], args["trig"], args["k"], args.get("values"))
            assert e.value.code == code and what in str(e.value), str(e.value)
        g.untouched()
        with pytest.raises(PgError) as e:                                # NULL outputs
            ctx.hot_recall_dev(hot, ref.GROUP, [[1]], 4, 0, 0)
        assert e.value.code == INVALID
        # the context serves the next call
        outs, _ = recall_dev(ctx, g, hot, ref.GROUP, [[cases.T_65]], 70)
        g.fetch()
        ref.same(outs, tuple(w[4:5] for w in cases.expected("group_wave_edges")))
    finally:
        g.free()


def test_upload_refusals_leave_the_table_unchanged(ctx):
    t = pa.Table(ctx, cases.ROWS, cases.DIM, 0)
    hot = ctx.hottable_create(t, 8)
    try:
        ok = (np.array([0, 2, 3], np.uint64), np.array([1, 1, 3], np.uint32), np.array([1.0, 0.0, 2.0]), np.array([0, 0x80, 5], np.uint8))
        hot.upload(*ok, trig0=1)
        before = hot.info()
        assert before["pairs"] == 3 and before["triggers_uploaded"] == 3
        want = ref.recall(cases.ROWS, 0, np.array([0, 0, 2, 3, 3, 3, 3, 3, 3], np.uint64), *ok[1:], ref.GROUP, [[2, 1, 0, 5]], 5)
        for name, tab in sorted(cases.bad_uploads().items()):
            with pytest.raises(PgError) as e:
                hot.upload(*tab, trig0=4)
            assert e.value.code == INVALID, name
            assert hot.info() == before, name
            ref.same(ctx.hot_recall(hot, ref.GROUP, [[2, 1, 0, 5]], 5), want)
        for trig0, n in ((2, 2), (7, 2), (9, 0)):                         # behind the last upload; past the table's end
            with pytest.raises(PgError) as e:
                hot.upload(np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0), np.zeros(0, np.uint8), trig0=trig0)
            assert e.value.code == INVALID and hot.info() == before
        hot.upload(*ok, trig0=6)                                          # 3 .. 5 skipped: empty; the arrays grow
        assert hot.info() == dict(before, pairs=6, triggers_uploaded=8)
        ref.same(ctx.hot_recall(hot, ref.GROUP, [[7, 4, 1, 6]], 8),
                 ref.recall(cases.ROWS, 0, np.array([0, 0, 2, 3, 3, 3, 3, 5, 6], np.uint64), *(np.concatenate([a, a]) for a in ok[1:]), ref.GROUP,
                            [[7, 4, 1, 6]], 8))
    finally:
        hot.destroy()
        t.destroy()


def test_stale_generation_and_views(ctx):
    rng = np.random.default_rng(3)
    t = pa.Table(ctx, 1000, cases.DIM, 50)
    other = pa.Table(ctx, 1000, cases.DIM, 50)
    t.upload(rng.standard_normal((1000, cases.DIM)).astype(np.float32))
    hot = ctx.hottable_create(t, 2)
    try:
        hot.upload(np.array([0, 2, 2], np.uint64), np.array([5, 999], np.uint32), np.array([1.0, 2.0]), np.array([0, 1], np.uint8))
        got = ctx.hot_recall(hot, ref.GROUP, [[0]], 3)
        assert got[0][0].tolist() == [50 + 999, 50 + 5, ref.PAD_ROW] and got[3][0] == 2
        # a filtered view has no hot table: its rows are not the source's
        feats = pa.Features(ctx, 1000)
        feats.set_column("c", pa.F_I32, (np.arange(1000) % 3).astype(np.int32))
        view = t.view(feats, "c", "==", 1)
        try:
            with pytest.raises(PgError) as e:
                pa.HotTable(ctx, view, 2)
            assert e.value.code == INVALID and "a filtered view has no hot table" in str(e.value)
        finally:
            view.destroy()
            feats.destroy()
        t.swap(other)
        with pytest.raises(PgError) as e:
            ctx.hot_recall(hot, ref.GROUP, [[0]], 3)
        m = re.search(r"generation (\d+) of its item table, which is at generation (\d+) \(stale\)", str(e.value))
        assert e.value.code == INVALID and m and int(m.group(1)) == hot.info()["generation"] and int(m.group(2)) > int(m.group(1))
        with pytest.raises(PgError) as e:
            pa.HotTable(ctx, t, 0)
        assert e.value.code == INVALID
    finally:
        hot.destroy()
        other.destroy()
        t.destroy()


def test_chained_into_the_fan_in_without_a_synchronisation(ctx, base):
    """pg_hot_recall_dev, then pg_fanin_merge_dev over its answer and a second fixed list, enqueued back to back: one
    synchronisation at the end.  A refused call stands between two such chains and changes nothing."""
    _, hot = base
    rng = np.random.default_rng(8)
    nq, k, k2 = 5, 96, 40
    trig = [[cases.T_65, cases.T_ONE], [], [cases.T_1025], [cases.T_SOURCES, cases.T_TIE_C], [cases.T_8193]]
    seed = [3, 4, 5, 6, 7]
    off, rows, sc, src = cases.table()[1]
    fixed_rows = (cases.ROW_OFFSET + rng.integers(0, cases.ROWS, (nq, k2))).astype(np.uint64)
    for q in range(nq):                                                  # some ids the hot answer holds too, some padding
        fixed_rows[q, :5] = cases.ROW_OFFSET + rows[int(off[cases.T_65]):int(off[cases.T_65]) + 5]
    fixed_rows[:, -3:] = ref.PAD_ROW
    fixed_sc = rng.standard_normal((nq, k2)).astype(np.float32)
    g = Guarded(ctx)
    try:
        d_fr, d_fs = g.put(fixed_rows), g.put(fixed_sc)
        chains = []
        for mode in (ref.GROUP, ref.GLOBAL):
            outs, d = recall_dev(ctx, g, hot, mode, trig, k, None, seed)
            cap = k + k2
            merged = [np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.float64), np.empty((nq, cap), np.uint8),
                      np.empty((2, nq, cap), np.float64), np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)]
            ctx.fanin_merge_dev([(d[0], d[1], k, True), (d_fr, d_fs, k2, False)], nq, *[g.out(a) for a in merged])
            chains.append((mode, outs, merged))
            if mode == ref.GROUP:
                with pytest.raises(PgError):
                    ctx.hot_recall_dev(hot, ref.GROUP, cases.TOO_LONG[0][0], k, d[0], d[1], d[2], d[3])
        g.fetch()
        for mode, outs, merged in chains:
            want = ref.recall(cases.ROWS, cases.ROW_OFFSET, off, rows, sc, src, mode, trig, k, None, seed)
            ref.same(outs, want)
            fanin_ref.same(merged, fanin_ref.merge([(want[0], want[1]), (fixed_rows, fixed_sc)]))
    finally:
        g.free()
