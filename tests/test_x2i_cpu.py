"""The U2I2X2I recall without a GPU: tests/x2i_ref.py against exact rationals and hand-worked answers, and
pg_x2i_recall_host (csrc/x2i_host.hpp through the library) against x2i_ref.py, bit for bit, on those cases and on the GPU tests' grid."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import x2i_cases as cases
import x2i_ref as ref
import pairec_amd as pa
from pairec_amd import _lib
from pairec_amd._lib import PgError


def assert_same(got, want):
    assert np.array_equal(np.asarray(got[2], np.uint32), np.asarray(want[2], np.uint32))
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))


def tiny(rows, n_x, i2x, x2i, row_offset=0):
    """{row: [x]}, {x: [(item, score)]} → XLists"""
    xl = ref.XLists(rows, n_x, row_offset)
    for r, xs in i2x.items():
        xl.upload_item2x([0, len(xs)], xs, r)
    for x, l in x2i.items():
        xl.upload_x2item([0, len(l)], [i for i, _ in l], [s for _, s in l], x)
    return xl


def host(xl, trig, pref, k, normalize=True, max_rule=False, lists=None):
    return pa.x2i_recall_host(xl.rows, xl.row_offset, xl.n_x, *xl.csr(), trig, pref, k, normalize, max_rule, lists)


def both(xl, trig, pref, k, normalize=True, max_rule=False, lists=None):
    """the restatement's answer, after pg_x2i_recall_host gave the same"""
    want = ref.x2i_recall(xl, trig, pref, k, normalize, max_rule, lists)
    assert_same(host(xl, trig, pref, k, normalize, max_rule, lists), want)
    return want


# ---- the restatement against exact arithmetic ----------------------------------------------------------------------------------------

def exact(xl, trig, pref, max_rule=False):
    """item -> Fraction, by the definition, in exact rationals (sums do not depend on the order there)"""
    xp = {}
    for r, p in zip(trig, pref):
        for x in xl.i2x.get(int(r), ()):
            xp[x] = xp.get(x, 0) + Fraction(p)
    out = {}
    for x, p in xp.items():
        for item, s in zip(*xl.x2i.get(x, ((), ()))):
            if item in set(trig):
                continue
            t = p * Fraction(s)
            if item not in out:
                out[item] = t
            elif max_rule:
                out[item] = max(out[item], t)
            else:
                out[item] += t
    return out


def test_restatement_against_exact_rationals():
    rng = np.random.default_rng(1)
    rows, n_x = 40, 8
    i2x = {r: rng.choice(n_x, int(rng.integers(0, 4)), replace=False).tolist() for r in range(rows)}
    i2x[0], i2x[1] = [3, 5], [5, 3]                              # an X shared by triggers
    x2i = {x: [(int(i), float(s)) for i, s in zip(rng.choice(rows, 12, replace=False), rng.choice([0.25, 0.5, 0.75, 1.0, 1.5, 2.0], 12))]
           for x in range(n_x)}
    xl = tiny(rows, n_x, i2x, x2i, 100)
    trig, pref = [0, 1, 7, 9, 12], [1, 2, 3, 4, 1]
    for max_rule in (False, True):
        ex = exact(xl, trig, pref, max_rule)
        assert len(ex) > 10 and max(ex.values()) > 0
        got = both(xl, [trig], [pref], 40, False, max_rule)
        assert got[2][0] == len(ex)
        for row, s in zip(got[0][0][:len(ex)], got[1][0]):
            assert Fraction(float(s)) == ex[int(row) - 100]         # dyadic scores, small integers: every float operation was exact
        order = sorted(ex.items(), key=lambda kv: (-kv[1], kv[0]))   # ties in row order
        assert [int(r) - 100 for r in got[0][0][:len(ex)]] == [i for i, _ in order]
        assert len(set(ex.values())) < len(ex)
    # m a power of two: the division is exact as well
    xl = tiny(10, 2, {0: [0], 1: [1]}, {0: [(5, 1.0), (6, 0.5)], 1: [(5, 1.0), (7, 0.25), (6, 0.5)]})
    got = both(xl, [[0, 1]], [[3, 5]], 5, True)
    assert list(got[0][0][:3]) == [5, 6, 7] and list(got[1][0][:3]) == [1.0, 0.5, 0.15625] and got[2][0] == 3


def test_addition_order_of_both_hops():
    big = [1e16, 1.0, -1e16]
    # hop 1: three triggers onto one X — (1e16 + 1) - 1e16 loses the 1, (1e16 - 1e16) + 1 keeps it
    xl = tiny(10, 1, {0: [0], 1: [0], 2: [0]}, {0: [(5, 1.0)]})
    got = both(xl, [[0, 1, 2], [0, 2, 1]], [big, [big[0], big[2], big[1]]], 2, False)
    assert got[1][0][0] == 0.0 and got[1][1][0] == 1.0
    # hop 2: the same three terms onto one item through three X, in the X's order of first appearance
    xl = tiny(10, 3, {0: [2], 1: [0], 2: [1]}, {0: [(5, 1.0)], 1: [(5, 1.0)], 2: [(5, 1.0)]})
    got = both(xl, [[0, 1, 2], [0, 2, 1]], [big, [big[0], big[2], big[1]]], 2, False)
    assert got[1][0][0] == 0.0 and got[1][1][0] == 1.0


def test_first_appearance_order_is_not_x_id_order():
    xl = tiny(10, 3, {0: [2, 0], 1: [1]}, {2: [(5, 1.0)], 0: [(5, 1.0)], 1: [(5, 1.0)]})
    assert [x for x, _ in ref.hop1(xl, [0, 1], [1.0, 2.0])] == [2, 0, 1]
    xl = tiny(10, 3, {0: [2], 1: [0], 2: [1]}, {2: [(5, 1e16)], 0: [(5, -1e16)], 1: [(5, 1.0)]})
    got = both(xl, [[0, 1, 2]], [[1.0, 1.0, 1.0]], 2, False)
    assert got[1][0][0] == 1.0                                       # (1e16 - 1e16) + 1; in id order (-1e16 + 1) + 1e16 = 0


def hand_worked():
    # four triggers 0 .. 3 (prefer 2, 1, 3, 1) and three X: A = 2, B = 0, C = 1 by id
    A, B, C = 2, 0, 1
    i2x = {0: [A], 1: [A, B], 2: [B, C], 3: [C]}
    x2i = {A: [(10, 0.5), (0, 1.0), (11, 1.0)], B: [(11, 0.25), (12, 1.0)], C: [(10, 0.5), (3, 2.0), (13, 0.25)]}
    return tiny(20, 3, i2x, x2i, 1000), [0, 1, 2, 3], [2.0, 1.0, 3.0, 1.0]


def test_hand_worked_collaborative_path():
    """xPrefer: A = 2 + 1 = 3, B = 1 + 3 = 4, C = 3 + 1 = 4 (user_collaborative_u2i2x2i_hologres_dao.go:196-211).  Rows of A, B, C with
    triggers 0 and 3 skipped (:311-315): 10: 1.5 + 2.0, 11: 3.0 + 1.0, 12: 4.0, 13: 1.0.  m = 4 (mergeUserCollaborativeItemsResult)."""
    xl, trig, pref = hand_worked()
    assert ref.hop1(xl, trig, pref) == [(2, 3.0), (0, 4.0), (1, 4.0)]
    got = both(xl, [trig], [pref], 6, True)
    assert list(got[0][0]) == [1011, 1012, 1010, 1013, ref.U64MAX, ref.U64MAX]
    assert list(got[1][0]) == [1.0, 1.0, 0.875, 0.25, -np.inf, -np.inf] and got[2][0] == 4
    got = both(xl, [trig], [pref], 6, False)
    assert list(got[1][0][:4]) == [4.0, 4.0, 3.5, 1.0]
    # the realtime path keeps the largest entry: 10: max(1.5, 2.0), 11: max(3.0, 1.0)
    got = both(xl, [trig], [pref], 3, False, True)
    assert list(got[0][0]) == [1012, 1011, 1010] and list(got[1][0]) == [4.0, 3.0, 2.0] and got[2][0] == 3
    got = both(xl, [trig], [pref], 6, True, True)                    # max_rule ignores normalize
    assert list(got[1][0][:4]) == [4.0, 3.0, 2.0, 1.0]


def test_a_skipped_trigger_would_have_been_the_maximum():
    xl, trig, pref = hand_worked()
    with_it = both(xl, [trig[:3]], [pref[:3]], 6, True)              # without trigger 3: C = 3, item 3 scores 6.0 and is the maximum
    assert with_it[0][0][0] == 1003 and with_it[1][0][0] == 1.0
    skipped = both(xl, [trig[:3] + [3]], [pref[:3] + [0.0]], 6, True)   # the same sums, item 3 now a trigger
    assert 1003 not in list(skipped[0][0])
    rows = list(with_it[0][0][1:with_it[2][0]])
    assert rows == list(skipped[0][0][:skipped[2][0]])
    assert np.all(skipped[1][0][:3] > with_it[1][0][1:4])            # every normalised score changed: m fell from 6 to 4


def test_max_rule_with_signed_zeros():
    xl = tiny(10, 2, {0: [0], 1: [1]}, {0: [(5, 1.0)], 1: [(5, 1.0)]})
    got = both(xl, [[0, 1], [1, 0]], [[0.0, -0.0], [-0.0, 0.0]], 1, False, True)
    # the first term stays: a later one replaces it only when it is LARGER, and 0.0 > -0.0 is false either way
    assert not np.signbit(got[1][0][0]) and np.signbit(got[1][1][0])
    xl = tiny(10, 2, {0: [0], 1: [1]}, {0: [(5, 1.0), (6, 1.0)], 1: [(4, 1.0)]})
    got = both(xl, [[0, 1]], [[-0.0, 0.0]], 3, True)                 # -0.0 ranks as 0.0: row order, bits kept
    assert list(got[0][0]) == [4, 5, 6] and list(np.signbit(got[1][0])) == [False, True, True]


def test_non_finite_x_sum_is_dropped():
    xl = tiny(10, 2, {0: [0, 1], 1: [0], 2: [1]}, {0: [(5, 1.0)], 1: [(6, 1.0)]})
    got = both(xl, [[0, 1, 2]], [[1e308, 1e308, -1e308]], 3, False)
    assert got[2][0] == 1 and got[0][0][0] == 6 and got[1][0][0] == 0.0
    got = both(xl, [[0, 1], [0, 2]], [[1e308, 1e308], [1e308, -1e308]], 3, False)
    assert list(got[2]) == [1, 2]


def test_exclusion_lists_on_the_host():
    xl, trig, pref = hand_worked()
    got = both(xl, [trig, trig], [pref, pref], 2, True, False, [[1011, 5, 1000], []])
    assert list(got[0][0]) == [1012, 1010] and list(got[0][1]) == [1011, 1012]


# ---- the grid of the GPU tests ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    built = cases.build()
    xl = ref.XLists(cases.ROWS, cases.N_X, cases.ROW_OFFSET)
    cases.upload(xl, built)
    return xl, xl.csr()


@pytest.mark.parametrize("name", sorted(cases.grid()))
def test_host_statement_on_the_gpu_grid(table, name):
    xl, arrays = table
    trig, pref, k, normalize, max_rule = cases.grid()[name]
    got = pa.x2i_recall_host(xl.rows, xl.row_offset, xl.n_x, *arrays, trig, pref, k, normalize, max_rule)
    assert_same(got, ref.x2i_recall(xl, trig, pref, k, normalize, max_rule))


def test_host_statement_limits(table):
    xl, arrays = table
    many = list(range(cases.R_MANY, cases.R_MANY + 17))
    assert ref.limit(xl, many[:16], np.ones(16)) is None and ref.limit(xl, many, np.ones(17)) == "x"
    full = list(range(cases.R_LONG, cases.R_LONG + 64))
    assert ref.limit(xl, full, np.ones(64)) is None and ref.limit(xl, full + [cases.R_ONE], np.ones(65)) == "pairs"
    for trig, word in ((many, "distinct X"), (full + [cases.R_ONE], "pairs")):
        with pytest.raises(PgError) as e:
            pa.x2i_recall_host(xl.rows, xl.row_offset, xl.n_x, *arrays, [[cases.R_WIDE], [], trig, trig],
                               [[1.0], [], np.ones(len(trig)), np.ones(len(trig))], 50)
        assert e.value.code == -4 and "request 2" in str(e.value) and word in str(e.value)


# ---- refusals that need no device --------------------------------------------------------------------------------------------------------

def test_argument_refusals():
    xl, trig, pref = hand_worked()

    def code(*a, **kw):
        with pytest.raises(PgError) as e:
            host(xl, *a, **kw)
        return e.value.code
    assert code([], [], 5) == -1                                     # nq = 0
    assert code([[0]] * 257, [[1.0]] * 257, 5) == -1
    assert code([[0]], [[1.0]], 0) == -4 and code([[0]], [[1.0]], 16385) == -4
    assert code([np.zeros(257, np.uint32)], [np.ones(257)], 5) == -4
    assert code([[0]], [[np.nan]], 5) == -1 and code([[0]], [[np.inf]], 5) == -1
    assert code([[0]], [[1.0]], 5, lists=[np.arange(4097)]) == -4
    assert code([[0]], [[1.0]], 16384 - 4095, lists=[np.arange(4096)]) == -4
    host(xl, [[0]], [[1.0]], 16384 - 4096, lists=[np.arange(4096)])


def test_hostile_csr_is_refused():
    one = np.ones(3, np.float32)
    good = ([0, 1, 2, 2], [0, 1], [0, 3, 3], [1, 0, 2], one)

    def code(i2x_off, i2x_ids, x2i_off, x2i_rows, x2i_scores, rows=3, n_x=2):
        with pytest.raises(PgError) as e:
            pa.x2i_recall_host(rows, 0, n_x, i2x_off, i2x_ids, x2i_off, x2i_rows, x2i_scores, [[0]], [[1.0]], 3)
        return e.value.code
    pa.x2i_recall_host(3, 0, 2, *good, [[0]], [[1.0]], 3)
    assert code([0, 2, 1, 2], [0, 1], *good[2:]) == -1                                # offsets descend
    assert code([0, 1, 2, 2], [0, 2], *good[2:]) == -1                                # an x id >= n_x
    assert code([0, 2, 2, 2], [1, 1], *good[2:]) == -1                                # an x id twice
    assert code(*good[:2], [0, 3, 3], [1, 3, 0], one) == -1                           # an item row >= rows
    assert code(*good[:2], [0, 3, 3], [1, 0, 2], [1.0, np.inf, 1.0]) == -1            # a non-finite score
    assert code(*good[:2], [0, 3, 3], [1, 0, 2], [1.0, 1.0, np.nan]) == -1
    assert code(*good[:2], [0, 2, 3], [1, 1, 0], one) == -1                           # an item twice in one list
    assert code([0, 65, 65], np.arange(65), [0] * 67, [], [], 2, 66) == -1            # an item's X list longer than 64
    pa.x2i_recall_host(2, 0, 66, [0, 64, 64], np.arange(64), [0] * 67, [], [], [[0]], [[1.0]], 3)
    assert code([0] * 1027, [], [0, 1025], np.arange(1025), np.ones(1025), 1026, 1) == -1   # an X's item list longer than 1024
    pa.x2i_recall_host(1026, 0, 1, [0] * 1027, [], [0, 1024], np.arange(1024), np.ones(1024), [[0]], [[1.0]], 3)


def test_upload_entry_points_refuse_without_a_context():
    L = _lib.load()
    off = np.zeros(2, np.uint64)
    assert L.pg_xtable_upload_item2x(None, None, 0, 1, off.ctypes.data_as(C.c_void_p), None) == -1
    assert L.pg_xtable_upload_x2item(None, None, 0, 1, off.ctypes.data_as(C.c_void_p), None, None) == -1
    assert L.pg_xtable_create(None, None, 5, None) == -1
    assert L.pg_xtable_info(None, None, None, None, None, None) == -1
    assert L.pg_x2i_recall(None, None, None, None, None, 1, 1, None, None, None, None) == -1
    assert L.pg_rtu2i_x_recall(None, None, None, None, None, None, None, None, None, 1, 1, None, None, None, None) == -1
