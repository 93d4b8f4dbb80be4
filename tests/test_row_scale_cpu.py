"""CPU tests of the row-scale cases (tests/row_scale_cases.py): the reference alone meets every precondition the GPU tests of
tests/test_gpu_row_scale.py rely on — group, chunk and trip counts, the 3-row last block, which masks the compact path may serve,
where the duplicate pairs lie — for devices of 64, 256 and 304 CUs; and at the 256-CU row count the host mirrors the GPU tests use
as references are held to numpy: pg_where_eval_host of every compound clause word for word, pg_cold_recall_host against
tests/coldstart_ref.py.  No GPU is used."""
import functools

import numpy as np
import pytest

import coldstart_ref as ref
import pairec_amd as pa
import row_scale_cases as cases
from row_scale_cases import BLOCK, G

CUS = (64, 256, 304)


@functools.lru_cache(maxsize=2)
def world(rows, cus):
    return cases.masks(rows, cus), cases.store(rows, cus)


@functools.lru_cache(maxsize=1)
def order_columns(rows):
    return cases.order_columns(rows)


def test_row_count_at_256_cus():
    assert cases.rows_for(256) == 4_199_427 == cases.rows_for(64)          # (below 256 CUs the five groups decide)
    assert cases.rows_for(304) == (16 * 304 + 5) * 1024 + 3


@pytest.mark.parametrize("cus", CUS)
def test_shape(cus):
    rows = cases.rows_for(cus)
    s = cases.shape(rows, cus)
    assert s["blocks"] == max(16 * cus, 4096) + 6
    assert s["groups"] == 5 and s["blocks"] % 1024 != 0                    # thread 1 of the totals' scan holds group 4, a partial one
    assert rows > 4 * G + 1                                                # (the issue's 4 194 305 rows)
    assert s["grid"] == 8 * cus and s["blocks"] > 2 * s["grid"] and s["blocks"] % s["grid"] != 0      # two full trips, a ragged last
    assert s["trips"] >= 3 and (cus < 256 or s["trips"] == 3)
    assert s["last_block_rows"] == 3 and rows % 4 == 3 and rows % 32 == 3
    for n in (rows - 3, 8 * cus * BLOCK + 1):                              # the bitmap tests' other two row counts
        assert n < rows
    assert (rows - 3) % BLOCK == 0
    assert cases.shape(8 * cus * BLOCK + 1, cus)["trips"] == 2 and cases.shape(8 * cus * BLOCK, cus)["trips"] == 1


@pytest.mark.parametrize("cus", CUS)
def test_masks(cus):
    rows = cases.rows_for(cus)
    s = cases.shape(rows, cus)
    m, cols = world(rows, cus)
    assert tuple(m) == cases.MASKS
    per_block = {name: np.add.reduceat(mask.astype(np.int64), np.arange(0, rows, BLOCK)) for name, mask in m.items()}
    per_group = {name: np.add.reduceat(pb, np.arange(0, s["blocks"], 1024)) for name, pb in per_block.items()}
    for name in ("edges", "sparse") + (("last_group",) if cus <= 256 else ()):       # (a device above 256 CUs has a longer last group)
        assert 0 < int(m[name].sum()) * 8 <= rows, name                   # the compact path may serve them
    for name in ("eighth", "one_group"):                                   # ... and not these: a whole group of five is one row in four
        assert rows < int(m[name].sum()) * 8 and int(m[name].sum()) <= (8 << 20) // 2, name      # ("where_compact_min_ratio" keeps them in place)
    assert int(m["edges"].sum()) == 1 + 3 + 2 * cases.EDGE * (s["groups"] - 1)
    for g in range(1, s["groups"]):                                        # both sides of every group boundary, the first row, the last three
        assert m["edges"][g * G - cases.EDGE:g * G + cases.EDGE].all() and not m["edges"][g * G + cases.EDGE] and not m["edges"][g * G - cases.EDGE - 1]
    assert m["edges"][0] and m["edges"][-3:].all() and not m["edges"][1] and not m["edges"][-4]
    assert per_group["one_group"].tolist() == [0, 0, 0, 1 << 20, 0]
    assert per_group["last_group"].tolist() == [0, 0, 0, 0, rows - 4 * G] and 0 < rows - 4 * G < G
    assert set(per_block["sparse"][:-1].tolist()) == {1, 2} and per_block["sparse"][-1] in (0, 1) and (per_group["sparse"] > 0).all()
    assert (per_group["eighth"] > 0).all() and (per_block["eighth"][:-1] > 0).all()
    tail = np.flatnonzero(m["trip_tail"])
    assert tail.size and tail[0] == 2 * s["trip_rows"] and tail.size == rows - 2 * s["trip_rows"]      # nothing of the first two trips
    if cus >= 256:
        assert tail[-1] // s["trip_rows"] == 2                             # ... and the third is the last
    assert not m["none"].any() and m["all"].all()
    # every mask again from the store's columns, as its clause states it; the flag columns
    for name, (_, in_numpy) in cases.clauses(rows, cus).items():
        got = in_numpy(cols)
        assert got.dtype == np.bool_ and np.array_equal(got, m[name]), name
        assert cols["f_" + name].dtype == np.int32 and np.array_equal(cols["f_" + name] == 1, m[name])
        assert cols["g_" + name].dtype == np.int64 and np.array_equal(cols["g_" + name] == cases.BIG + 1, m[name])
        assert int(cols["g_" + name].min()) >= cases.BIG


@pytest.mark.parametrize("cus", CUS)
def test_duplicate_pairs_and_the_table(cus):
    rows = cases.rows_for(cus)
    m, _ = world(rows, cus)
    p1, p2 = cases.dup_pairs(m["eighth"])
    assert p1 == (G - 1, G) and p2[0] < G - 1 and p2[1] > G and len({*p1, *p2}) == 4
    assert m["edges"][list(p1 + p2)].all()                                # `edges` admits both pairs
    assert m["eighth"][list(p2)].all() and not m["eighth"][p2[0] + 1:G - 1].any() and not m["eighth"][G + 1:p2[1]].any()
    ids = np.flatnonzero(m["eighth"])
    at = np.searchsorted(ids, p2[0])
    assert ids[at + 1 + int(m["eighth"][G - 1]) + int(m["eighth"][G])] == p2[1]       # neighbours in the compaction but for the first pair
    assert not m["one_group"][list(p1 + p2)].any()
    if cus != 256:
        return
    tab = cases.table(rows, m["eighth"])
    assert tab.dtype == np.float32 and tab.shape == (rows, cases.DIM)
    assert np.array_equal(cases.decode(tab), np.arange(rows))             # every row names itself
    for (a, b), val in zip((p1, p2), cases.PAIR_VALUES):
        assert np.array_equal(tab[a, 2:], tab[b, 2:]) and (tab[a, 2:10] == np.float32(val)).all()
    others = np.ones(rows, bool)
    others[list(p1 + p2)] = False
    assert np.abs(tab[others, 2:10]).max() <= 1.0 and not tab[:, 10:].any()
    q = cases.queries()
    assert q.shape == (cases.NQ_MAX, cases.DIM) and not q[:, :2].any() and (q[0, 2:10] == 1.0).all()
    # query 0's inner products: the pairs' 16 and 14 above every other row's (<= 8), so they lead wherever they are admitted
    assert float(tab[p1[0], 2:10] @ q[0, 2:10]) == 16.0 and float(tab[p2[0], 2:10] @ q[0, 2:10]) == 14.0


def test_where_eval_host_equals_numpy():
    rows = cases.rows_for(256)
    m, cols = world(rows, 256)
    for name, (clause, _) in cases.clauses(rows, 256).items():
        w = pa.Where(clause)
        assert len(w.columns) >= 2, (name, w.columns)                     # compound: never the single-column form
        dts = {cols[c].dtype.type for c in w.columns}
        assert dts == {np.int32, np.int64}, (name, dts)
        for n in (rows, rows - 3, 8 * 256 * BLOCK + 1):
            host = w.eval_host({c: cols[c][:n] for c in w.columns}, n)
            assert np.array_equal(host, cases.bitmap(m[name][:n])), (name, n)
        w.free()


@pytest.mark.parametrize("pool", ("edges", "eighth"))
def test_cold_recall_host_equals_the_restatement(pool):
    rows = cases.rows_for(256)
    m, _ = world(rows, 256)
    bits = cases.bitmap(m[pool])
    two = order_columns(rows)["i32_two"]
    seeds = np.array([0, (1 << 64) - 1, 0x123456789ABCDEF0], np.uint64)
    for order_by, direction in ((None, None), ("i32_two ASC", "asc"), ("i32_two desc", "desc")):
        c = pa.ColdStart(None, order_by)
        for k in (7, 16384):
            got = c.recall_host(rows, 3, k, bits=bits, seed=seeds, order_col=None if order_by is None else two, row_offset=cases.ROW_OFFSET)
            want = ref.recall(direction, bits, rows, 3, k, col=two, seed=seeds, row_offset=cases.ROW_OFFSET)
            ref.same(got, want, "pool %s order %s k %d" % (pool, order_by, k))
        c.free()


def test_i32_two_runs_cross_the_chunk_boundaries():
    """what the ordered GPU cases rely on: ascending at depth 16 384 over every row, the better rows and the threshold's ties span
    chunks 0 .. 2 and the cut falls behind the third boundary; over the sparse pool at depth 4 096 the cut falls in the last full group"""
    rows = cases.rows_for(256)
    m, _ = world(rows, 256)
    two = order_columns(rows)["i32_two"]
    low = np.flatnonzero(two == -3)
    assert low[16383] >= 3 * G - cases.TWO_RUN and low.size > 16384
    sp = np.flatnonzero(m["sparse"])
    n_low = int((two[sp] == -3).sum())
    assert 0 < n_low < 4096 < sp.size and sp[two[sp] == 11][4096 - n_low - 1] >= 3 * G
    assert (np.bincount(sp[two[sp] == -3] >> 20, minlength=5)[:4] > 0).all()
