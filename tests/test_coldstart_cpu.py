"""CPU tests of ColdStartRecall's host side (include/pairec_gpu.h "ColdStartRecall"; csrc/coldstart_host.hpp): the OrderBy parser,
pg_cold_recall_host against the independent restatement of tests/coldstart_ref.py on the device tests' grid, the three stated
consequences of the permutation (distinct ids, a permutation of the pool at k >= A, the prefix property) and its uniformity over
the fixed seeds 0 .. 19 999 with numpy's own permutation through the same check as the control.  No GPU is used."""
import numpy as np
import pytest

import coldstart_cases as cases
import coldstart_ref as ref
import pairec_amd as pa
from pairec_amd import _lib

N_SEEDS = 20000


def _cold(order_by=None, where=None):
    return pa.ColdStart(where, order_by)


# ---- the parser -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [None, "", "   ", "random()", "RANDOM()", " Random ( ) ", "\trandom()\n"])
def test_order_by_random_forms(text):
    c = _cold(text)
    got = c.recall_host(5, 1, 5)                      # (a random order needs no column)
    assert sorted(got[0][0].tolist()) == list(range(5))
    c.free()


@pytest.mark.parametrize("text, desc", [("create_time", False), ("create_time ASC", False), ("create_time asc", False),
                                        ("  create_time   DeSc  ", True), ("_x9 desc", True), ("random", False), ("random asc", False)])
def test_order_by_column_forms(text, desc):
    c = _cold(text)
    col = np.array([3, 1, 2, 5, 4], np.int32)
    got = c.recall_host(5, 2, 3, order_col=col)
    want = [3, 4, 0] if desc else [1, 2, 0]
    assert got[0].tolist() == [want, want] and got[2].tolist() == [3, 3]
    with pytest.raises(_lib.PgError) as e:            # an ordered pool needs its column
        c.recall_host(5, 1, 3)
    assert e.value.code == -1
    c.free()


@pytest.mark.parametrize("text, pos", [("a, b", 1), ("a,b", 1), ("a + 1", 2), ("a DESC NULLS FIRST", 7), ("a ASC, b", 5), ("1a", 0),
                                       ("random(1)", 7), ("random(", 7), ("a b", 2), ("a desc desc", 7), ("-a", 0), ("(a)", 0),
                                       ("a;", 1), ("random() desc", 9), ("a\x01", 1), ("\xc3\xa9", 0), ("a.b", 1), ("a DESCx", 2)])
def test_order_by_refusals_name_the_position(text, pos):
    with pytest.raises(_lib.PgError) as e:
        _cold(text)
    assert e.value.code == -6, str(e.value)           # PG_ERR_PARSE
    assert str(e.value).endswith("at position %d" % pos), str(e.value)


def test_create_and_host_argument_checks():
    L = _lib.load()
    assert L.pg_cold_create(None, None, None) == -1
    c = _cold()
    r, s, n = np.zeros(4, np.uint64), np.zeros(4, np.float32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data                      # noqa: E731
    assert L.pg_cold_recall_host(c.h, None, 4, 0, None, 0, None, 0, 1, p(r), p(s), p(n)) == -1       # nq = 0
    assert L.pg_cold_recall_host(c.h, None, 4, 0, None, 0, None, 257, 1, p(r), p(s), p(n)) == -1
    assert L.pg_cold_recall_host(c.h, None, 4, 0, None, 0, None, 1, 0, p(r), p(s), p(n)) == -4       # k = 0: PG_ERR_UNSUPPORTED
    assert L.pg_cold_recall_host(c.h, None, 4, 0, None, 0, None, 1, 16385, p(r), p(s), p(n)) == -4
    assert L.pg_cold_recall_host(c.h, None, 1 << 32, 0, None, 0, None, 1, 1, p(r), p(s), p(n)) == -4
    assert L.pg_cold_recall_host(c.h, None, 4, 0, None, 0, None, 1, 4, None, p(s), p(n)) == -1
    assert L.pg_cold_recall_host(c.h, None, 4, 0, None, 0, None, 1, 4, p(r), p(s), None) == 0         # the counts are optional
    assert sorted(r.tolist()) == [0, 1, 2, 3]
    c.free()


# ---- the host statement against the restatement ---------------------------------------------------------------------------------
def test_vector_permutation_equals_the_python_ints():
    for A in (1, 2, 3, 4, 5, 16, 17, 64, 65, 1000, 65536, 65537, 300001):
        for seed in (0, 1, (1 << 64) - 1, 0x123456789ABCDEF0):
            n = min(A, 40)
            assert ref.perm_np(seed, A, n).tolist() == [ref.perm(seed, A, i) for i in range(n)], (A, seed)


@pytest.mark.parametrize("rows", cases.ROWS)
def test_random_order_equals_the_restatement(rows):
    cols, masks = cases.store(rows), cases.masks(rows)
    rng = np.random.default_rng(rows)
    c = _cold()
    for pool, clause in cases.POOLS.items():
        bits = None
        if clause is not None:
            w = pa.Where(clause)
            bits = w.eval_host(cols, rows)
            w.free()
            assert np.array_equal(bits, cases.bitmap(masks[pool])), pool
        for k in cases.KS:
            nq = 3 if k <= 4096 else 1
            seed = np.array([0, 1, (1 << 64) - 1], np.uint64)[:nq] if k % 2 else rng.integers(0, 1 << 63, nq).astype(np.uint64) * np.uint64(2) + np.uint64(1)
            for sd in (seed, None):
                got = c.recall_host(rows, nq, k, bits=bits, seed=sd, row_offset=5 if k == 7 else 0)
                ref.same(got, ref.recall(None, bits, rows, nq, k, seed=sd, row_offset=5 if k == 7 else 0), "rows %d pool %s k %d" % (rows, pool, k))
    c.free()


@pytest.mark.parametrize("rows", (1, 33, 1025, 40000))
def test_ordered_equals_the_restatement(rows):
    masks, ocols = cases.masks(rows), cases.order_columns(rows)
    for (dn, pattern), col in ocols.items():
        for direction in ("asc", "desc"):
            c = _cold("v " + direction)
            for pool in ("all_null", "third", "dense_sparse", "none"):
                bits = None if pool == "all_null" else cases.bitmap(masks[pool])
                A = int(masks[pool].sum())
                for k in sorted({1, 7, 256, 4096, 16384, min(max(A, 1), 16384), min(A + 1, 16384)}):
                    got = c.recall_host(rows, 2, k, bits=bits, order_col=col, seed=[3, 4], row_offset=9)
                    ref.same(got, ref.recall(direction, bits, rows, 2, k, col=col, row_offset=9),
                             "rows %d %s %s %s pool %s k %d" % (rows, dn, pattern, direction, pool, k))
            c.free()


def test_nan_order_is_postgres():
    """every NaN equal and greater than every number: first under DESC, last under ASC; ties (the NaNs, the zeros) by row"""
    col = np.array([1.0, np.nan, -0.0, np.inf, 0.0, -np.inf], np.float32)
    col[1:2].view(np.uint32)[0] = 0xFFC00001          # a negative-signed NaN with a payload
    col = np.concatenate([col, np.array([np.nan], np.float32)])
    c = _cold("v")
    assert c.recall_host(7, 1, 7, order_col=col)[0][0].tolist() == [5, 2, 4, 0, 3, 1, 6]
    c.free()
    c = _cold("v desc")
    assert c.recall_host(7, 1, 7, order_col=col)[0][0].tolist() == [1, 6, 3, 0, 2, 4, 5]
    c.free()


# ---- the three consequences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, pool", [(1, "all_null"), (33, "third"), (1025, "tail"), (40000, "dense_sparse"), (40000, "all_true")])
def test_ids_are_distinct_and_cover_the_pool(rows, pool):
    mask = cases.masks(rows)[pool]
    members = np.flatnonzero(mask)
    A = len(members)
    c = _cold()
    seeds = np.array([0, 1, (1 << 64) - 1, 0xDEADBEEF], np.uint64)
    for k in (1, 7, 256, min(A, 16384), min(A + 1, 16384)):
        r, _, n = c.recall_host(rows, 4, k, bits=cases.bitmap(mask), seed=seeds)
        for q in range(4):
            ids = r[q, :n[q]].tolist()
            assert n[q] == min(k, A) and len(set(ids)) == len(ids) and set(ids) <= set(members.tolist())
            if k >= A:
                assert sorted(ids) == members.tolist()          # a permutation of the pool
    c.free()


@pytest.mark.parametrize("k", (1, 7, 256))
def test_answer_is_a_prefix_of_any_deeper_answer(k):
    rows = 40000
    c = _cold()
    seeds = np.array([0, 1, (1 << 64) - 1, 77], np.uint64)
    for pool in ("third", "dense_sparse", "tail"):
        bits = cases.bitmap(cases.masks(rows)[pool])
        deep = c.recall_host(rows, 4, 4096, bits=bits, seed=seeds)
        shallow = c.recall_host(rows, 4, k, bits=bits, seed=seeds)
        n = int(shallow[2][0])
        assert n == min(k, int(deep[2][0])) and np.array_equal(shallow[0][:, :n], deep[0][:, :n])
    c.free()


# ---- uniformity (deterministic: the seeds are fixed) ----------------------------------------------------------------------------
def _answers(A: int, k: int):
    """[N_SEEDS][k]: the answers of seeds 0 .. N_SEEDS - 1 over a pool of every row of A"""
    c = _cold()
    out = np.empty((N_SEEDS, k), np.int64)
    for s in range(0, N_SEEDS, 250):
        out[s:s + 250] = c.recall_host(A, 250, k, seed=np.arange(s, s + 250, dtype=np.uint64))[0].astype(np.int64)
    c.free()
    return out


def _control(A: int, k: int):
    rng = np.random.default_rng(12345)
    return np.stack([rng.permutation(A)[:k] for _ in range(N_SEEDS)])


def _chi2(counts: np.ndarray, expected: float) -> float:
    return float(((counts - expected) ** 2 / expected).sum())


@pytest.mark.parametrize("draw", (_answers, _control), ids=("library", "numpy"))
def test_marginals_are_uniform(draw):
    A, k = 64, 8
    a = draw(A, k)
    limit = ref.chi2_quantile_999(A - 1)
    anyslot = _chi2(np.bincount(a.reshape(-1), minlength=A), N_SEEDS * k / A)
    slot0 = _chi2(np.bincount(a[:, 0], minlength=A), N_SEEDS / A)
    print("A=64 k=8: any-slot chi2 %.1f, slot-0 chi2 %.1f, 0.999 quantile %.1f" % (anyslot, slot0, limit))
    assert anyslot < limit and slot0 < limit


@pytest.mark.parametrize("A", (3, 10, 17, 50))
@pytest.mark.parametrize("draw", (_answers, _control), ids=("library", "numpy"))
def test_first_two_slots_are_jointly_uniform(draw, A):
    a = draw(A, 2)
    assert (a[:, 0] != a[:, 1]).all()
    cells = np.bincount(a[:, 0] * A + a[:, 1], minlength=A * A).reshape(A, A)
    off = cells[~np.eye(A, dtype=bool)]
    limit = ref.chi2_quantile_999(A * (A - 1) - 1)
    stat = _chi2(off, N_SEEDS / (A * (A - 1)))
    print("A=%d: pair chi2 %.1f, 0.999 quantile %.1f" % (A, stat, limit))
    assert stat < limit
