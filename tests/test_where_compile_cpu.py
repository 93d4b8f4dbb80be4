"""CPU tests of the compound WhereClause compiler (pg_where_compile): pg_where_eval_host — the compiled program
on host arrays, which is what the device kernel reproduces — equals a numpy mask for every form of the grammar; every refused
form is PG_ERR_PARSE with the position in the message; every limit passes at the limit and fails one beyond; hostile nesting is
an error, not a stack overflow.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib

PARSE = -6
ROWS = 1003            # not a multiple of 32
BIG = 1 << 33


def cols(seed=5, n=ROWS):
    rng = np.random.default_rng(seed)
    c = {"a": rng.integers(-6, 7, n).astype(np.int32), "b": rng.integers(-6, 7, n).astype(np.int64),
         "c": rng.integers(0, 5, n).astype(np.int32), "status": rng.integers(0, 3, n).astype(np.int32),
         "big": BIG + rng.integers(-50, 50, n).astype(np.int64) * 7919,
         "create_time": rng.integers(0, 1000, n).astype(np.int32), "cat_id": rng.integers(0, 20, n).astype(np.int32),
         "stock": rng.integers(-2, 3, n).astype(np.int64), "_x9": rng.integers(-3, 4, n).astype(np.int32)}
    m = min(n, 4)
    c["a"][:m] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0, -1][:m]
    c["b"][:m] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1][:m]
    return c


def unpack(bits, n):
    r = np.arange(n)
    return ((bits[r >> 5] >> (r & 31).astype(np.uint32)) & 1).astype(bool)


def compile_rc(clause):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.pg_where_compile(clause.encode(), C.byref(h))
    msg = L.pg_last_error().decode() if rc else ""
    if rc == 0:
        L.pg_where_free(h)
    return rc, msg


def check(clause, ref, c=None):
    c = c or cols()
    n = len(c["a"])
    w = pa.Where(clause)
    try:
        got = w.eval_host(c)
    finally:
        w.free()
    assert got.shape == ((n + 31) // 32,)
    assert np.array_equal(unpack(got, n), ref), clause
    # the tail of the last word stays zero
    if n % 32:
        assert int(got[-1]) >> (n % 32) == 0, clause


def test_every_operator_spelling_equals_numpy():
    c = cols()
    a, b = c["a"], c["b"]
    for sp, f in ((">", np.greater), (">=", np.greater_equal), ("<", np.less), ("<=", np.less_equal), ("=", np.equal), ("==", np.equal),
                  ("!=", np.not_equal), ("<>", np.not_equal)):
        for v in (-7, -1, 0, 3, 6, 2**31 - 1, -2**31):
            check("a %s %d" % (sp, v), f(a.astype(np.int64), v), c)
            check("b%s%d" % (sp, v), f(b, v), c)
    # the ends of long long: > MAX and < MIN admit nothing, >= MIN and <= MAX everything
    mx, mn = 2**63 - 1, -2**63
    check("b > %d" % mx, np.zeros(ROWS, bool), c)
    check("b < %d" % mn, np.zeros(ROWS, bool), c)
    check("b >= %d" % mn, np.ones(ROWS, bool), c)
    check("b <= %d" % mx, np.ones(ROWS, bool), c)
    check("b = %d" % mn, b == mn, c)
    check("b != %d" % mx, b != mx, c)
    check("a = +3", a == 3, c)


def test_precedence_not_and_parentheses():
    c = cols()
    a, b, cc = c["a"].astype(np.int64), c["b"], c["c"]
    check("a = 1 OR b = 2 AND c = 3", (a == 1) | ((b == 2) & (cc == 3)), c)
    check("(a = 1 OR b = 2) AND c = 3", ((a == 1) | (b == 2)) & (cc == 3), c)
    check("a = 1 AND b = 2 OR c = 3", ((a == 1) & (b == 2)) | (cc == 3), c)
    check("NOT a = 1 AND b > 0", ~(a == 1) & (b > 0), c)                      # NOT binds tighter than AND
    check("NOT (a = 1 AND b > 0)", ~((a == 1) & (b > 0)), c)
    check("NOT NOT a > 2", a > 2, c)
    check("NOT (a > 2 OR NOT (b < 0 AND NOT c = 1))", ~((a > 2) | ~((b < 0) & ~(cc == 1))), c)
    check("((((a >= -1)))) and (((b <= 1)) or ((c <> 0)))", (a >= -1) & ((b <= 1) | (cc != 0)), c)
    check("a > 0 or (b > 0 and (c > 0 or (a < -2 and (b < -2 or c = 4))))",
          (a > 0) | ((b > 0) & ((cc > 0) | ((a < -2) & ((b < -2) | (cc == 4))))), c)
    check("(a > 0 and b > 0) or (a < 0 and b < 0) or (c = 2 and (a = 0 or b = 0))",
          ((a > 0) & (b > 0)) | ((a < 0) & (b < 0)) | ((cc == 2) & ((a == 0) | (b == 0))), c)
    # a balanced tree of 64 terms: the deepest evaluation stack the compiler can be asked for
    level = ["a %s %d" % ((">", "<")[i % 2], (i % 11) - 5) for i in range(32)] + ["b %s %d" % (("<=", ">=")[i % 2], (i % 9) - 4) for i in range(32)]
    vals = [(a > (i % 11) - 5) if i % 2 == 0 else (a < (i % 11) - 5) for i in range(32)] + \
           [(b <= (i % 9) - 4) if i % 2 == 0 else (b >= (i % 9) - 4) for i in range(32)]
    depth = 0
    while len(level) > 1:
        op = ("AND", "OR")[depth % 2]
        level = ["(%s %s %s)" % (level[i], op, level[i + 1]) for i in range(0, len(level), 2)]
        vals = [(vals[i] & vals[i + 1]) if depth % 2 == 0 else (vals[i] | vals[i + 1]) for i in range(0, len(vals), 2)]
        depth += 1
    check(level[0], vals[0], c)
    check("NOT " + level[0], ~vals[0], c)


def test_in_between_constants_and_keyword_case():
    c = cols()
    a, b, big = c["a"].astype(np.int64), c["b"], c["big"]
    check("a IN (3)", a == 3, c)
    check("a IN (5, -2, 5, 0, -2, 3, 3)", np.isin(a, [5, -2, 0, 3]), c)           # duplicates, unsorted
    check("a NOT IN (5, -2, 5, 0)", ~np.isin(a, [5, -2, 0]), c)
    check("NOT a IN (1, 2)", ~np.isin(a, [1, 2]), c)
    check("NOT a NOT IN (1, 2)", np.isin(a, [1, 2]), c)
    check("b in (%d, %d, 0)" % (2**63 - 1, -2**63), np.isin(b, [2**63 - 1, -2**63, 0]), c)
    check("a BETWEEN -2 AND 3", (a >= -2) & (a <= 3), c)                          # both bounds inclusive
    check("a BETWEEN 3 AND 3", a == 3, c)
    check("a BETWEEN 3 AND -2", np.zeros(ROWS, bool), c)                          # an empty range
    check("a NOT BETWEEN 3 AND -2", np.ones(ROWS, bool), c)
    check("a NOT BETWEEN -1 AND 1 AND b BETWEEN -3 AND 3", ~((a >= -1) & (a <= 1)) & ((b >= -3) & (b <= 3)), c)
    check("a BETWEEN -1 AND 1 OR b = 2", ((a >= -1) & (a <= 1)) | (b == 2), c)     # BETWEEN's AND is not the connective
    some = [int(v) for v in np.unique(big)[::7]]
    check("big > %d" % (BIG + 7919 * 10), big > BIG + 7919 * 10, c)               # int64 constants beyond 2^32
    check("big IN (%s)" % ", ".join(map(str, some[::-1])), np.isin(big, some), c)
    check("big between %d and %d and a < 0" % (BIG - 7919 * 5, BIG + 7919 * 5), (big >= BIG - 7919 * 5) & (big <= BIG + 7919 * 5) & (a < 0), c)
    check("a > -4 AnD b < -1 oR nOt a iN (1,2) aNd b BeTwEeN -3 aNd 3", ((a > -4) & (b < -1)) | (~np.isin(a, [1, 2]) & (b >= -3) & (b <= 3)), c)
    check("status = 1 AND create_time > 500", (c["status"] == 1) & (c["create_time"] > 500), c)
    check("cat_id IN (3, 7, 12) AND stock > 0", np.isin(c["cat_id"], [3, 7, 12]) & (c["stock"] > 0), c)
    check("\t_x9\n>=\r 0   and _x9<2", (c["_x9"] >= 0) & (c["_x9"] < 2), c)
    # an IN list of 1024 constants (the limit), against a column that hits about half of them
    rng = np.random.default_rng(9)
    wide = {"a": rng.integers(0, 4096, ROWS).astype(np.int32)}
    lst = rng.permutation(4096)[:1024]
    check("a in (%s)" % ",".join(map(str, lst)), np.isin(wide["a"], lst), wide)


def test_row_counts_around_a_word():
    for n in (1, 31, 32, 33, 63, 64, 65, 1024, 1025):
        c = cols(seed=n, n=n)
        check("a > 0 AND b < 3 OR c IN (1, 4)", ((c["a"] > 0) & (c["b"] < 3)) | np.isin(c["c"], [1, 4]), c)


def test_columns_are_deduplicated_in_first_appearance_order():
    L = _lib.load()
    w = pa.Where("zeta > 1 AND alpha IN (1,2) OR zeta < -1 AND NOT (beta BETWEEN 1 AND 2 OR alpha = 7)")
    assert w.columns == ["zeta", "alpha", "beta"]
    assert L.pg_where_num_columns(w.h) == 3
    assert L.pg_where_column_name(w.h, 3) is None and L.pg_where_column_name(w.h, -1) is None
    w.free()
    assert L.pg_where_compile(None, None) == -1                                   # PG_ERR_INVALID
    assert L.pg_where_num_columns(None) == 0


@pytest.mark.parametrize("clause,pos", [
    ("a = 'x'", 4), ("a = \"x\"", 4), ("a = 1.5", 5), ("a = 1e5", 5), ("abs(a) > 1", 3), ("a + 1 > 2", 2), ("a > 1 b", 6),
    ("a > 1 AND", 9), ("a > 1 OR OR b = 1", 9), ("", 0), ("   ", 3), ("a", 1), ("a >", 3), ("a > b", 4), ("1 > a", 0),
    ("a > 9223372036854775808", 4), ("a < -9223372036854775809", 4), ("a in (1, 99999999999999999999)", 9),
    ("(a > 1", 6), ("a > 1)", 5), ("a in ()", 6), ("a in (1,)", 8), ("a in 1", 5), ("a in (1 2)", 8), ("a not > 1", 6),
    ("a between 1", 11), ("a between 1 or 2", 12), ("a between 1 and", 15), ("a ! 1", 2), ("a => 1", 3), ("a > - 1", 4),
    ("not", 3), ("and a = 1", 0), ("a = 1 and in (1)", 10), ("a.b = 1", 1), ("a = 1;", 5), ("a is null", 2), ("a like 1", 2),
])
def test_refused_forms_are_parse_errors_with_the_position(clause, pos):
    rc, msg = compile_rc(clause)
    assert rc == PARSE, (clause, rc)
    assert msg.endswith("at position %d" % pos), (clause, msg)


def test_each_limit_passes_at_the_limit_and_fails_one_beyond():
    def terms(n, ncols=1):
        return " AND ".join("c%d > %d" % (i % ncols, i) for i in range(n))

    assert compile_rc(terms(16, 16))[0] == 0                                     # 16 distinct columns
    rc, msg = compile_rc(terms(17, 17))
    assert rc == PARSE and "columns" in msg and "at position" in msg
    assert compile_rc(terms(64))[0] == 0                                         # 64 terms
    rc, msg = compile_rc(terms(65))
    assert rc == PARSE and "terms" in msg and "at position" in msg
    lists = lambda sizes: " OR ".join("a IN (%s)" % ",".join(map(str, range(s))) for s in sizes)
    assert compile_rc(lists([1024]))[0] == 0                                     # 1024 IN constants in total
    assert compile_rc(lists([1000, 24]))[0] == 0
    assert compile_rc(lists([512, 512]))[0] == 0
    for sizes in ([1025], [1000, 25], [1, 1024]):
        rc, msg = compile_rc(lists(sizes))
        assert rc == PARSE and "IN constants" in msg and "at position" in msg
    assert compile_rc("(" * 64 + "a = 1" + ")" * 64)[0] == 0                      # nesting depth 64
    assert compile_rc("NOT " * 64 + "a = 1")[0] == 0
    assert compile_rc("NOT (" * 32 + "a = 1" + ")" * 32)[0] == 0
    for clause in ("(" * 65 + "a = 1" + ")" * 65, "NOT " * 65 + "a = 1", "NOT (" * 32 + "(a = 1)" + ")" * 32):
        rc, msg = compile_rc(clause)
        assert rc == PARSE and "nesting" in msg and "at position" in msg
    # the limits together, evaluated: 16 columns, 64 terms
    rng = np.random.default_rng(3)
    c = {"c%d" % i: rng.integers(0, 64, 500).astype(np.int64 if i % 2 else np.int32) for i in range(16)}
    clause = " OR ".join("(c%d > %d AND c%d <= %d)" % (i % 16, 60 - i, (i + 5) % 16, i) for i in range(32))
    ref = np.zeros(500, bool)
    for i in range(32):
        ref |= (c["c%d" % (i % 16)] > 60 - i) & (c["c%d" % ((i + 5) % 16)] <= i)
    w = pa.Where(clause)
    assert len(w.columns) == 16
    assert np.array_equal(unpack(w.eval_host(c), 500), ref)
    w.free()


def test_hostile_nesting_is_an_error_not_a_stack_overflow():
    for clause in ("(" * 100_000, "(" * 100_000 + "a = 1" + ")" * 100_000, "NOT " * 100_000 + "a = 1", "NOT (" * 50_000 + "a = 1",
                   "a = 1" + " AND (b = 2" * 100_000):
        rc, msg = compile_rc(clause)
        assert rc == PARSE and "at position" in msg
    # length alone is no nesting: a long flat clause within the limits compiles
    assert compile_rc("a = 1" + " OR a = 2" * 63)[0] == 0
    assert compile_rc(" " * 200_000 + "a = 1")[0] == 0


def test_eval_host_argument_checks_and_stats_without_a_gpu():
    L = _lib.load()
    w = pa.Where("a > 1 AND b < 2")
    assert w.stats() == {"builds": 0, "hits": 0, "last_build_ms": 0.0, "bytes": 0, "epoch": 0, "admitted": 0}
    assert L.pg_where_eval_host(w.h, None, None, 4, None) == -1
    a = np.arange(4, dtype=np.int32)
    ptrs = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    out = np.zeros(1, np.uint32)
    assert L.pg_where_eval_host(w.h, ptrs, (C.c_int * 2)(pa.F_I32, pa.F_F32), 4, out.ctypes.data_as(C.c_void_p)) == -1
    assert b"int32 / int64" in L.pg_last_error()
    assert L.pg_where_eval_host(w.h, ptrs, (C.c_int * 2)(pa.F_I32, pa.F_I32), 4, out.ctypes.data_as(C.c_void_p)) == 0
    assert int(out[0]) == 0                            # a > 1 AND a < 2 admits nothing
    assert L.pg_where_stats(None, None) == -1
    assert L.pg_recall_topk_where_ex(None, None, None, None, 0, None, 1, 1, None, None, None) == -1
    assert L.pg_index_recall_topk_where_ex(None, None, None, None, 0, None, 1, 1, None, None, None) == -1
    assert L.pg_table_view_create_ex(None, None, None, None, None) == -1
    assert L.pg_where_bits(None, None, None, 0, None, None) == -1
    w.free()
