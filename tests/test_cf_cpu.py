"""CPU tests of the collaborative-filter recall's specification (tests/cf_ref.py) and of the ABI that serves it: the reference
against exact rationals, the addition order, a hand-worked example of the reference's own code path, and the exports."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import numpy as np

import cf_ref as ref
from pairec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_row_lists(rows, lists):
    """SimLists whose row r has the (neighbour, similarity) pairs lists[r]"""
    sl = ref.SimLists(rows)
    for r, pairs in lists.items():
        sl.upload([0, len(pairs)], [p[0] for p in pairs], [p[1] for p in pairs], row0=r)
    return sl


def test_reference_against_exact_rationals():
    # dyadic similarities, small-integer preferences: every product and every sum is exact in binary64
    lists = {
        0: [(10, 0.5), (11, 0.25), (12, 1.0), (13, 0.125)],
        1: [(11, 0.75), (10, 0.5), (14, 2.0)],
        2: [(12, 0.25), (15, 4.0), (13, 1.875)],
        3: [(16, 0.5)],
    }
    trig, pref = [0, 1, 2, 3, 1], [2, 3, 4, 16, 1]
    exact = {}
    for r, p in zip(trig, pref):
        for item, s in lists[r]:
            exact[item] = exact.get(item, Fraction(0)) + Fraction(s) * p
    # rows 10 and 12 tie at 3, rows 14 and 16 at 8
    assert exact[10] == exact[12] == 3 and exact[14] == exact[16] == 8
    m = max(exact.values())
    assert m == 16                                               # a power of two: the normalised scores are exact too
    sl = one_row_lists(20, lists)
    for normalize in (False, True):
        want = sorted(((i, s / m if normalize else s) for i, s in exact.items()), key=lambda kv: (-kv[1], kv[0]))
        rows, scores, counts = ref.cf_recall(sl, [trig], [pref], 16, normalize)
        n = len(want)
        assert counts[0] == n
        assert [int(x) for x in rows[0, :n]] == [i for i, _ in want]
        assert [Fraction(float(x)) for x in scores[0, :n]] == [s for _, s in want]
        assert np.all(rows[0, n:] == ref.U64MAX) and np.all(np.isneginf(scores[0, n:]))
        # ties are in row order
        ids = [int(x) for x in rows[0, :n]]
        assert ids.index(10) + 1 == ids.index(12) and ids.index(14) + 1 == ids.index(16)


def test_reference_addition_order():
    # three triggers contribute 1e16, 1.0 and -1e16 to one item: (1e16 + 1.0) - 1e16 is 0.0 in binary64, not 1.0
    sl = one_row_lists(8, {0: [(5, 1.0)], 1: [(5, 1.0)], 2: [(5, 1.0)]})
    rows, scores, counts = ref.cf_recall(sl, [[0, 1, 2]], [[1e16, 1.0, -1e16]], 2, normalize=False)
    assert counts[0] == 1 and rows[0, 0] == 5
    assert scores[0, 0] == 0.0
    # ... and in another order it is not
    _, scores, _ = ref.cf_recall(sl, [[0, 2, 1]], [[1e16, -1e16, 1.0]], 2, normalize=False)
    assert scores[0, 0] == 1.0


def test_reference_worked_example():
    with open(os.path.join(ROOT, "tests", "golden", "cf_known_answer.json")) as f:
        g = json.load(f)
    row = g["item_rows"]
    name = {v: k for k, v in row.items()}
    sl = ref.SimLists(len(row))
    for item, text in g["similar_item_ids"].items():
        pairs = [s.split(":") for s in text.split(",")]
        sl.upload([0, len(pairs)], [row[p[0]] for p in pairs], [float(p[1]) for p in pairs], row0=row[item])
    trig, pref = [], []
    for s in g["user_item_ids"].split(","):
        parts = s.split(":")
        trig.append(row[parts[0]])
        pref.append(float(parts[1]) if len(parts) > 1 else 1.0)      # a missing preference is 1
    for key, normalize in (("normalization_off", False), ("normalization_on", True)):
        rows, scores, counts = ref.cf_recall(sl, [trig], [pref], 5, normalize)
        want = g["expected"][key]
        n = len(want["ids"])
        assert counts[0] == n
        assert [name[int(x)] for x in rows[0, :n]] == want["ids"]
        assert [float(x) for x in scores[0, :n]] == want["scores"]


def test_library_exports_the_cf_entry_points():
    names = ["pg_simtable_create", "pg_simtable_upload", "pg_cf_recall", "pg_cf_recall_dev"]
    L = C.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "pairec_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", src))
    for n in names:
        assert hasattr(L, n), n
        assert n in declared, n
    # host-side argument checks need no device
    L = _lib.load()
    assert L.pg_cf_recall(None, None, None, None, None, 1, 1, None, None, None, None) == -1
    assert L.pg_simtable_upload(None, None, 0, 0, None, None, None) == -1
    assert L.pg_simtable_info(None, None, None, None, None) == -1
