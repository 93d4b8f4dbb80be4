"""CPU tests of the recalls with per-request exclusion lists: the header declares the new entries and the
built library exports them; tests/exclude_ref.py — the numpy restatement every GPU expectation comes from — equals an oracle
recall over the table with the excluded rows physically removed, ids mapped back."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exclude_ref as ref
from oracle import oracle as o
from pairec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("pg_exclude_compact_dev", "pg_recall_topk_exclude", "pg_recall_topk_exclude_dev", "pg_i2i_recall_exclude",
         "pg_coalescer_recall_exclude")


def test_header_declares_and_library_exports_the_six_symbols():
    src = open(os.path.join(ROOT, "include", "pairec_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\}\s*pg_recall_exclude_opts\s*;", src)          # the options struct
    L = C.CDLL(_lib.LIB_PATH)
    for name in FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert C.sizeof(_lib.PgRecallExcludeOpts) == 8 + 2 * C.sizeof(C.c_void_p)


def test_null_arguments_are_invalid_without_a_device():
    L = _lib.load()
    assert L.pg_exclude_compact_dev(None, None, None, 1, 1, None, None, 1, 0.0, None, None, None) == -1
    assert L.pg_recall_topk_exclude(None, None, None, 1, 1, None, None, None, None, None, None) == -1
    assert L.pg_recall_topk_exclude_dev(None, None, None, 1, 1, None, None, None, None, None, None) == -1
    assert L.pg_i2i_recall_exclude(None, None, None, 1, None, 1, 0, None, None, None, None, None) == -1
    assert L.pg_coalescer_recall_exclude(None, None, None, 0, None, None, None) == -1
    # fs without where
    opts = _lib.PgRecallExcludeOpts(0, C.c_void_p(8), None)
    assert L.pg_recall_topk_exclude(None, None, None, 1, 1, None, None, C.byref(opts), None, None, None) == -1
    assert b"come together" in L.pg_last_error()


def removed_rows_oracle(tab, q, k, ids, l2, row_offset):
    """the oracle over the table WITHOUT the rows `ids` (global), local rows of the smaller table mapped back"""
    keep = np.ones(tab.shape[0], bool)
    local = np.asarray(ids, np.int64) - row_offset
    local = local[(local >= 0) & (local < tab.shape[0])]
    keep[local] = False
    left = np.flatnonzero(keep)
    rows = np.full(k, ref.U64MAX, np.uint64)
    sc = np.full(k, np.inf if l2 else -np.inf, np.float32)
    n = min(k, left.size)
    if n:
        orow, osc = (o.recall_topk_l2 if l2 else o.recall_topk)(tab[left], q.reshape(1, -1), k)
        rows[:n] = left[orow[0].astype(np.int64)].astype(np.uint64) + np.uint64(row_offset)
        sc[:n] = osc[0]
    return rows, sc, n


@pytest.mark.parametrize("dim", [64, 128])
@pytest.mark.parametrize("l2", [False, True])
def test_restatement_equals_the_oracle_without_the_rows(dim, l2):
    n, k, off = 3000, 40, 7_000_000
    rng = np.random.default_rng(5 + dim + l2)
    tab = o.synth_rows(o.SEED_TABLE, 0, n, dim) * rng.uniform(0.8, 1.2, (n, 1)).astype(np.float32)
    q = o.synth_rows(o.SEED_QUERY, 0, 6, dim)
    lists = []
    for i, m in enumerate((0, 1, 17, 300, 40, 5)):
        top, _ = ref.plain_top(tab, q[i], k + m, l2, off)
        ids = rng.choice(top, m, replace=False) if m else np.zeros(0, np.uint64)
        lists.append(ids)
    # duplicates, UINT64_MAX, a row outside the table and an id below row_offset change nothing
    lists[3] = np.concatenate([lists[3], lists[3][:9], [ref.U64MAX, np.uint64(off + n + 5), np.uint64(3)]]).astype(np.uint64)
    got = ref.recall_exclude(tab, q, k, lists, l2, off)
    for i in range(6):
        want = removed_rows_oracle(tab, q[i], k, lists[i], l2, off)
        assert np.array_equal(got[0][i], want[0]), i
        assert np.array_equal(got[1][i].view(np.uint32), want[1].view(np.uint32)), i
        assert got[2][i] == want[2] == k


@pytest.mark.parametrize("l2", [False, True])
def test_restatement_on_tied_rows_and_k_beyond_the_survivors(l2):
    n, dim, k = 400, 64, 30
    tab = o.synth_rows(o.SEED_TABLE, 0, n, dim)
    tab[1::2] = tab[0::2]                          # every row twice: each score is a tie of rows 2i, 2i + 1
    q = o.synth_rows(o.SEED_QUERY, 3, 2, dim)
    top, sc = ref.plain_top(tab, q[0], k, l2)
    assert np.array_equal(sc[0::2].view(np.uint32), sc[1::2].view(np.uint32)) and np.all(top[0::2] + 1 == top[1::2])
    # one of a tied pair: the first of the best pair, the second of the next, both of the third
    lists = [np.array([top[0], top[3], top[4], top[5]], np.uint64), np.zeros(0, np.uint64)]
    got = ref.recall_exclude(tab, q, k, lists, l2)
    for i in range(2):
        want = removed_rows_oracle(tab, q[i], k, lists[i], l2, 0)
        assert np.array_equal(got[0][i], want[0]) and np.array_equal(got[1][i].view(np.uint32), want[1].view(np.uint32))
    assert got[0][0][0] == top[1] and got[0][0][1] == top[2] and got[0][0][2] == top[6]
    # k larger than the rows that survive: the count, then padding
    k2 = n - 10
    lists2 = [np.arange(0, 50, dtype=np.uint64), np.arange(100, 103, dtype=np.uint64)]
    got2 = ref.recall_exclude(tab, q, k2, lists2, l2)
    assert got2[2].tolist() == [n - 50, k2]
    for i in range(2):
        want = removed_rows_oracle(tab, q[i], k2, lists2[i], l2, 0)
        assert np.array_equal(got2[0][i], want[0]) and np.array_equal(got2[1][i].view(np.uint32), want[1].view(np.uint32))
        assert got2[2][i] == want[2]
    assert np.all(got2[0][0][n - 50:] == ref.U64MAX) and np.all(np.isinf(got2[1][0][n - 50:]))
