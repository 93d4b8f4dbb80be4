"""The > 128-query int8 screen on v_mfma_i32_16x16x64_i8 (csrc/recall.hip, the query halves of screen_kernel, its hit
records and screen_decode_kernel): every recall through pa.Table.recall_topk against the CPU oracle, ids, order and score
bits exact.  The dot products of the screen are exact integers, so a wrong answer here is a wrong lane -> (row, query)
mapping, a wrong operand layout or a lost record, never rounding."""
import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

D = 128
N0 = 40_000                      # 1 250 whole 32-row blocks


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def unit_rows(rng, n):
    x = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def check(t, tab, q, k, sel=None):
    rows, sc, cnt = t.recall_topk(q, k)
    assert t.screen_info()[0] == 1, "the table left the int8 shadow: the test no longer reaches the kernel it is about"
    idx = np.arange(len(q)) if sel is None else np.asarray(sel)
    orow, osc = o.recall_topk(tab, q[idx], k)
    assert cnt.tolist() == [min(k, len(tab))] * len(q)
    assert np.array_equal(rows[idx], orow)
    assert np.array_equal(bits(sc[idx]), bits(osc))
    assert rows.max() < len(tab)
    return rows


def test_a_winner_in_every_row_position_for_every_query():
    """Cover argument, checked below on the planted table itself (no GPU): for each of the 256 queries j a planted row sits
    at each of the 32 positions p of a block.  In the 16x16 output layout position p is row half p >> 4, lane group
    (p & 15) >> 2, register p & 3, and query j is query half j >> 7, column block (j >> 4) & 7, lane & 15 = j & 15: all
    32 x 256 (register, lane, column block, half) slots hold a true top-K row once."""
    _, _, plants = planted()
    seen = {(int(j), int(r % 32)) for j, r in plants}
    assert seen == {(j, p) for j in range(256) for p in range(32)}
    assert len({int(r) for _, r in plants}) == 256 * 32           # no two plants share a row


_planted = []


def planted():
    if not _planted:
        rng = np.random.default_rng(1601)
        tab = unit_rows(rng, N0)
        q = unit_rows(rng, 256)
        plants = []
        for j in range(256):
            for p in range(32):
                r = ((7 * j + 41 * p) % (N0 // 32)) * 32 + p
                # 1.5-1.8 x the norm of an ordinary row along the query: far above the ordinary rows' best (~0.4) for query j,
                # every plant of a query at its own score, elements <= ~0.3 (the shadow's scale stays that of a unit row's: int8)
                tab[r] = q[j] * np.float32(1.5 + 0.01 * p)
                plants.append((j, r))
        _planted.append((tab, q, plants))
    return _planted[0]


def test_every_lane_register_and_column_slot(ctx):
    tab, q, plants = planted()
    t = pa.Table(ctx, N0, D)
    t.upload(tab)
    k = 32
    rows = check(t, tab, q, k)
    for j in range(256):                                          # the answer of query j is exactly its 32 plants
        assert sorted(rows[j].tolist()) == sorted(r for jj, r in plants if jj == j)
    t.destroy()


_alone = []


def recalled_alone(ctx):
    """(table, queries, rows, scores of each of the 256 queries recalled alone) — computed once."""
    if not _alone:
        rng = np.random.default_rng(1602)
        tab = unit_rows(rng, N0 + 17)
        q = unit_rows(rng, 256)
        t = pa.Table(ctx, len(tab), D)
        t.upload(tab)
        k = 24
        r1 = np.empty((256, k), np.uint64)
        s1 = np.empty((256, k), np.float32)
        for i in range(256):
            r, s, _ = t.recall_topk(q[i:i + 1], k)
            r1[i], s1[i] = r[0], s[0]
        orow, osc = o.recall_topk(tab, q, k)
        assert np.array_equal(r1, orow) and np.array_equal(bits(s1), bits(osc))
        _alone.append((t, tab, q, k, r1, s1))
    return _alone[0]


@pytest.mark.parametrize("nq", [129, 143, 144, 145, 200, 255, 256])
def test_partly_filled_column_blocks_batching_invariance(ctx, nq):
    """The last 16-query column block in use is partly filled (129, 143, 145, 200, 255), just full (144, 256) or the second
    query half is nearly empty (129): every request equals the same query recalled alone, bit for bit."""
    t, tab, q, k, r1, s1 = recalled_alone(ctx)
    rows, sc, cnt = t.recall_topk(q[:nq], k)
    assert t.screen_info()[0] == 1
    assert cnt.tolist() == [k] * nq
    assert np.array_equal(rows, r1[:nq])
    assert np.array_equal(bits(sc), bits(s1[:nq]))


@pytest.mark.parametrize("tail", [1, 15, 16, 17, 31])
def test_ragged_last_block_with_the_best_rows_at_the_end(ctx, tail):
    """rows = tail (mod 32): the last block ends inside the first row half (1, 15), at its end (16), inside the second (17,
    31).  The best rows are among the last 40, so the answers come from the ragged block and the one before it, and no row
    past the end may be reported."""
    rng = np.random.default_rng(1603)
    n = N0 + tail
    tab = unit_rows(rng, n)
    u = unit_rows(rng, 1)[0]
    # every query leans towards u (cosine ~ 0.7) and so do the last 40 rows, at 1.5 x the norm: they score ~ 1 for every query,
    # an ordinary row at most ~ 0.5
    tail_rows = u[None, :] + np.float32(0.3) * unit_rows(rng, 40)
    tail_rows /= np.linalg.norm(tail_rows, axis=1, keepdims=True)
    tab[n - 40:] = tail_rows * (np.float32(1.5) + np.float32(0.01) * np.arange(40, dtype=np.float32)[:, None])
    q = unit_rows(rng, 256) + u[None, :]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = pa.Table(ctx, n, D)
    t.upload(tab)
    rows = check(t, tab, q, 16)
    assert np.all(rows >= n - 40)
    t.destroy()


def test_dense_hits_zero_query_and_heavy_ties(ctx):
    """A zero query among 256 (integer threshold <= 0: every row is its suspect) on a table of eight distinct rows repeated
    5 000 times each (every row ties with 4 999 others, ties go by row id): whole blocks of hit lanes in every column
    block, regions and the spill pool overflow, the plans fall back — the answers stay the oracle's."""
    rng = np.random.default_rng(1604)
    base = unit_rows(rng, 8)
    tab = np.ascontiguousarray(base[rng.integers(0, 8, N0 + 9)])
    q = unit_rows(rng, 256)
    q[5] = 0.0
    q[200] = 0.0
    q[17] = base[3]
    t = pa.Table(ctx, len(tab), D)
    t.upload(tab)
    check(t, tab, q, 50)
    t.destroy()


def test_dense_hits_table_in_ascending_score_order(ctx):
    """Every later row beats every earlier one for every query, K = 10, 256 queries: each bounded chunk of the last plan makes
    every row a suspect of every query — 16 column blocks x 64 lanes = 1 024 records per 32-row block, which the per-wave
    regions are sized for (recall_plan_math.hpp, floor_w)."""
    rng = np.random.default_rng(1605)
    n = 150_000
    v = unit_rows(rng, 1)[0]
    scale = np.linspace(0.2, 1.0, n, dtype=np.float32)[:, None]
    tab = (v[None, :] * scale + 0.002 * rng.standard_normal((n, D)).astype(np.float32)).astype(np.float32)
    q = (v[None, :] + 0.05 * rng.standard_normal((256, D)).astype(np.float32)).astype(np.float32)
    t = pa.Table(ctx, n, D)
    t.upload(tab)
    check(t, tab, q, 10)
    t.destroy()


def test_headline_k_with_256_queries(ctx):
    """K = 5 000, 256 queries, 150 K uniform rows: the headline's K at a size that runs in seconds."""
    rng = np.random.default_rng(1606)
    n = 150_000
    tab = unit_rows(rng, n)
    q = unit_rows(rng, 256)
    t = pa.Table(ctx, n, D)
    t.upload(tab)
    check(t, tab, q, 5000)
    t.destroy()
