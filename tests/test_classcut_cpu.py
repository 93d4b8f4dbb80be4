"""DiversityAdjustCountFilter without a GPU: the boolean front end and the two host statements of
csrc/classcut.hip against tests/classcut_ref.py — expression trees evaluated in Python, rendered to govaluate text for the
library — the refusals by name, the width, and the host mirror's config."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import classcut_ref as ref
import pairec_amd as pa
from pairec_amd import _lib
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX, ACC = pa.TRIM_FIX, pa.TRIM_ACCUMULATE
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
COLS = [("a", pa.F_I32), ("b", pa.F_I64), ("c", pa.F_F32), ("d", pa.F_F64)]
NAMES = [n for n, _ in COLS]
RECALLS = ["u2i", "hot", "i2i"]


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "pairec_gpu.h")).read()
    assert int(re.search(r"PG_ERR_INVALID\s*=\s*(-?\d+)", hdr).group(1)) == ERR_INVALID
    assert int(re.search(r"PG_ERR_UNSUPPORTED\s*=\s*(-?\d+)", hdr).group(1)) == ERR_UNSUPPORTED
    assert int(re.search(r"#define\s+PG_CLASSCUT_MAX_CLASSES\s+(\d+)", hdr).group(1)) == ref.MAX_CLASSES
    assert C.sizeof(_lib.PgClasscutRule) == 16 and _lib.PgClasscutRule.type.offset == 8 and _lib.PgClasscutRule.count.offset == 12


def hostile_columns(rng, n):
    """int32, int64, f32 and f64 columns with the values that break evaluators: NaN, ±inf, -0.0, int64 beyond 2^53"""
    a = rng.integers(-3, 5, n).astype(np.int32)
    a[rng.random(n) < 0.05] = np.int32(-2**31)
    b = rng.integers(-3, 5, n).astype(np.int64)
    big = rng.random(n) < 0.15
    b[big] = rng.choice(np.array([2**53 + 1, 2**53 + 2, -(2**53) - 1, 2**63 - 1, -2**63, 2**62 + 1], dtype=np.int64), int(big.sum()))
    c = rng.integers(-3, 5, n).astype(np.float32)
    c[rng.random(n) < 0.3] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.1, 2.5], dtype=np.float32), 1)[0]
    d = rng.integers(-3, 5, n).astype(np.float64)
    sp = rng.random(n) < 0.3
    d[sp] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.1, 2.5, 2.0**53 + 2], dtype=np.float64), int(sp.sum()))
    return {"a": a, "b": b, "c": c, "d": d}


def hostile_scores(rng, n):
    s = rng.integers(-2, 4, n).astype(np.float64)
    sp = rng.random(n) < 0.2
    s[sp] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.5]), int(sp.sum()))
    return s


def compile_trees(trees, rules=None):
    rules = rules or [(FIX, 1)] * len(trees)
    return pa.classcut_compile([(ref.render(t), ty, cnt) for t, (ty, cnt) in zip(trees, rules)], COLS, RECALLS)


# ---- masks ------------------------------------------------------------------------------------------------------------------

def test_masks_of_random_trees_equal_the_tree_evaluator():
    rng = np.random.default_rng(20240)
    n = 96
    for case in range(120):
        trees = []
        while len(trees) < int(rng.integers(1, ref.MAX_CLASSES + 1)):
            t = ref.random_bool_tree(rng, NAMES, RECALLS, int(rng.integers(0, 4)))
            ops, depth = ref.shape(t)
            if ops <= ref.MAX_OPS and depth <= ref.MAX_DEPTH:
                trees.append(t)
        cols = hostile_columns(rng, n)
        score = hostile_scores(rng, n)
        item_in = (rng.random(n) < 0.8).astype(np.uint8)           # candidates outside the store
        source = rng.integers(0, 5, n).astype(np.uint8)             # sources 3, 4 are >= n_recalls
        source[rng.random(n) < 0.05] = 0xFF
        cc = compile_trees(trees)
        try:
            got = pa.classcut_masks_host(cc, score, cols, item_in, source)
        finally:
            cc.free()
        want = ref.masks(trees, n, cols, item_in, score, source, RECALLS)
        assert np.array_equal(got, want), (case, [ref.render(t) for t in trees], np.flatnonzero(got != want)[:5])


def col(n):
    return ("col", n)


def num(v):
    return ("num", v)


PRECEDENCE = [
    ("a > 1 || b > 2 && c > 3", ("or", ("cmp", ">", col("a"), num(1)), ("and", ("cmp", ">", col("b"), num(2)), ("cmp", ">", col("c"), num(3))))),
    ("!(a > 1) && b == 2", ("and", ("not", ("cmp", ">", col("a"), num(1))), ("cmp", "==", col("b"), num(2)))),
    ("a + 1 > b * 2", ("cmp", ">", ("bin", "+", col("a"), num(1)), ("bin", "*", col("b"), num(2)))),
    ("-a ** 2 > 0", ("cmp", ">", ("bin", "**", ("neg", col("a")), num(2)), num(0))),
    ("a > 1 && b > 2 || c > 3", ("or", ("and", ("cmp", ">", col("a"), num(1)), ("cmp", ">", col("b"), num(2))), ("cmp", ">", col("c"), num(3)))),
    ("a - 1 - 2 > b / 2 / 2", ("cmp", ">", ("bin", "-", ("bin", "-", col("a"), num(1)), num(2)), ("bin", "/", ("bin", "/", col("b"), num(2)), num(2)))),
    ("a > 0 || b > 0 || c > 3 && d > 0", ("or", ("or", ("cmp", ">", col("a"), num(0)), ("cmp", ">", col("b"), num(0))),
                                          ("and", ("cmp", ">", col("c"), num(3)), ("cmp", ">", col("d"), num(0))))),
    ("[a] % 2 == 1 && a in (1, 3, -3)", ("and", ("cmp", "==", ("bin", "%", col("a"), num(2)), num(1)), ("in", col("a"), [1, 3, -3]))),
    ("!!(d >= 2.5)", ("not", ("not", ("cmp", ">=", col("d"), num(2.5))))),
    ("round(d / 2) <= recall_score", ("cmp", "<=", ("round", ("bin", "/", col("d"), num(2))), ("score",))),
]


@pytest.mark.parametrize("text,tree", PRECEDENCE, ids=[t for t, _ in PRECEDENCE])
def test_precedence_and_associativity(text, tree):
    rng = np.random.default_rng(7)
    n = 400
    cols = {k: rng.integers(-3, 5, n).astype(dt) for k, dt in zip(NAMES, (np.int32, np.int64, np.float32, np.float64))}
    score = rng.integers(-2, 4, n).astype(np.float64)
    cc = pa.classcut_compile([(text, FIX, 1)], COLS, RECALLS)
    got = pa.classcut_masks_host(cc, score, cols)
    cc.free()
    want = ref.masks([tree], n, cols, None, score, None, RECALLS)
    assert 0 < int(want.sum()) < n, "the data must decide"
    assert np.array_equal(got, want)


E, T, F = "a > -100", "recall_score > 0", "recall_score < 0"       # an error outside the store, true, false


@pytest.mark.parametrize("text,member", [
    ("%s && %s" % (E, T), False), ("%s && %s" % (T, E), False), ("%s && %s" % (E, E), False), ("%s && %s" % (T, T), True),
    ("%s || %s" % (E, T), False), ("%s || %s" % (T, E), True), ("%s || %s" % (E, E), False), ("%s || %s" % (F, T), True),
    ("%s || %s" % (F, E), False),
    # false && error is false, not an error: its negation is true; error && false stays an error under the negation
    ("!(%s && %s)" % (F, E), True), ("!(%s && %s)" % (E, F), False),
    ("!(%s || %s)" % (T, E), False), ("!(%s || %s)" % (E, T), False), ("!(%s || %s)" % (F, E), False),
    # an error propagates through arithmetic, comparators, in and !
    ("!(%s)" % E, False), ("(a + 1) in (1, 2) || %s" % T, False), ("recall_score + a * 0 == recall_score || %s" % T, False),
])
def test_short_circuit_error_rule(text, member):
    cc = pa.classcut_compile([(text, FIX, 1)], COLS, RECALLS)
    cols = {"a": np.array([1, 1], np.int32)}
    got = pa.classcut_masks_host(cc, np.array([1.0, 1.0]), cols, np.array([0, 1], np.uint8))
    cc.free()
    assert bool(got[0]) == member, text                      # the candidate outside the store
    inside = eval(text.replace("&&", " and ").replace("||", " or ").replace("!(", " not ("), {"a": 1, "recall_score": 1.0})
    assert bool(got[1]) == bool(inside), text                # the one inside: no error anywhere


def test_recall_name_forms():
    src = np.array([0, 1, 2, 3, 0xFF], np.uint8)             # 3 and 0xFF are >= n_recalls
    sc = np.zeros(5)
    for text, want in [("recall_name == 'hot'", [0, 1, 0, 0, 0]), ('recall_name != "hot"', [1, 0, 1, 1, 1]),
                       ("recall_name == 'nobody'", [0, 0, 0, 0, 0]), ("recall_name != 'nobody'", [1, 1, 1, 1, 1]),
                       ("recall_name in ('u2i', \"i2i\")", [1, 0, 1, 0, 0]), ("recall_name in ('nobody', 'hot')", [0, 1, 0, 0, 0]),
                       ("!(recall_name in ('u2i', 'hot', 'i2i'))", [0, 0, 0, 1, 1]), ("[recall_name] == 'u2i' && recall_score == 0", [1, 0, 0, 0, 0])]:
        cc = pa.classcut_compile([(text, FIX, 1)], COLS, RECALLS)
        assert cc.reads_recall_name
        got = pa.classcut_masks_host(cc, sc, source=src)
        with pytest.raises(PgError) as e:
            pa.classcut_masks_host(cc, sc)
        assert e.value.code == ERR_INVALID and "recall_name" in str(e.value)
        cc.free()
        assert got.tolist() == want, text
    cc = pa.classcut_compile([("a > 1", FIX, 1)], COLS, RECALLS)
    assert not cc.reads_recall_name
    cc.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

REFUSALS = [
    ("a > 1 ? 2 : 3", ERR_UNSUPPORTED, ["ternary"]), ("(a ?? 1) > 0", ERR_UNSUPPORTED, ["'??'"]),
    ("(a & 1) == 1", ERR_UNSUPPORTED, ["bitwise", "'&'"]), ("(a | 1) == 1", ERR_UNSUPPORTED, ["bitwise", "'|'"]),
    ("(a ^ 1) == 1", ERR_UNSUPPORTED, ["bitwise", "'^'"]), ("~a == 1", ERR_UNSUPPORTED, ["bitwise", "'~'"]),
    ("a << 1 > 2", ERR_UNSUPPORTED, ["bitwise", "'<<'"]), ("a >> 1 > 2", ERR_UNSUPPORTED, ["bitwise", "'>>'"]),
    ("recall_name =~ 'u2'", ERR_UNSUPPORTED, ["regex", "'=~'"]), ("recall_name !~ 'u2'", ERR_UNSUPPORTED, ["regex", "'!~'"]),
    ("true", ERR_UNSUPPORTED, ["boolean literal", "true"]), ("a > 1 && false", ERR_UNSUPPORTED, ["boolean literal", "false"]),
    ("(a > 1) == (b > 2)", ERR_UNSUPPORTED, ["'=='", "between bools"]), ("(a > 1) != (b > 2)", ERR_UNSUPPORTED, ["'!='", "between bools"]),
    ("recall_name > 'hot'", ERR_UNSUPPORTED, ["recall_name", "ordered comparisons"]),
    ("recall_name + 1 > 0", ERR_UNSUPPORTED, ["recall_name", "arithmetic"]),
    ("recall_name == 1", ERR_UNSUPPORTED, ["recall_name", "string literal only"]),
    ("a == 'hot'", ERR_UNSUPPORTED, ["string literal", "recall_name"]), ("'hot' == recall_name", ERR_UNSUPPORTED, ["string literal"]),
    ("recall_name == '2020-01-01'", ERR_UNSUPPORTED, ["string literal", "date"]),
    ("recall_name == 'two words'", ERR_UNSUPPORTED, ["string literal"]), ("recall_name == ''", ERR_UNSUPPORTED, ["string literal"]),
    ("a + 1", ERR_UNSUPPORTED, ["is a number, not a bool"]), ("recall_score", ERR_UNSUPPORTED, ["is a number, not a bool"]),
    ("(a > 1) + 1 > 0", ERR_UNSUPPORTED, ["a bool where a number is needed"]), ("!a", ERR_UNSUPPORTED, ["a number where a bool is needed"]),
    ("a && b > 1", ERR_UNSUPPORTED, ["a number where a bool is needed"]), ("a > 1 || b", ERR_UNSUPPORTED, ["a number where a bool is needed"]),
    ("a > 1 > 0", ERR_UNSUPPORTED, ["a bool where a number is needed"]), ("-(a > 1) > 0", ERR_UNSUPPORTED, ["a bool where a number is needed"]),
    ("a in (1)", ERR_UNSUPPORTED, ["one-element"]), ("recall_name in ('hot')", ERR_UNSUPPORTED, ["one-element"]),
    ("a in (1, b)", ERR_UNSUPPORTED, ["constant"]), ("a in (%s)" % ", ".join(str(i) for i in range(65)), ERR_UNSUPPORTED, ["65 values"]),
    ("sqrt(a) > 1", ERR_UNSUPPORTED, ["function", "sqrt"]), ("item.a > 1", ERR_UNSUPPORTED, ["accessor", "item.a"]),
    ("a ** 2 ** 2 > 1", ERR_UNSUPPORTED, ["chained '**'"]), ("(1, 2) == a", ERR_UNSUPPORTED, ["array"]),
    (" + ".join(["a"] * 33) + " > 0", ERR_UNSUPPORTED, ["operations"]),
    ("a + (a + (a + (a + (a + (a + (a + (a + (a + 1)))))))) > 0", ERR_UNSUPPORTED, ["depth"]),
    ("recall_name == 'hot", ERR_UNSUPPORTED, ["unterminated"]), ("(a > 1", ERR_UNSUPPORTED, ["missing ')'"]), ("", ERR_UNSUPPORTED, ["end of the expression"]),
    ("(" * 100 + "a > 1" + ")" * 100, ERR_UNSUPPORTED, ["nesting"]), ("a > 1e3", ERR_UNSUPPORTED, ["malformed number"]),
    ("zz > 1", ERR_INVALID, ['"zz"', "neither a declared column"]), ("u2i > 1", ERR_INVALID, ['"u2i"', "Properties"]),
]


@pytest.mark.parametrize("text,code,words", REFUSALS, ids=[t[:40] for t, _, _ in REFUSALS])
def test_expression_refusals_by_name(text, code, words):
    with pytest.raises(PgError) as e:
        pa.classcut_compile([(text, FIX, 1)], COLS, RECALLS)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    # the arithmetic front end keeps refusing all of it (a plain number is its own language)
    if "is a number, not a bool" not in words:
        with pytest.raises(PgError):
            pa.expr_compile_govaluate(text or "a >")


def test_more_than_sixteen_referenced_columns():
    cols = [("k%d" % i, pa.F_I32) for i in range(17)]
    ok = pa.classcut_compile([(" + ".join(n for n, _ in cols[:16]) + " > 0", FIX, 1)], cols, [])
    ok.free()
    with pytest.raises(PgError) as e:
        pa.classcut_compile([(" + ".join(n for n, _ in cols[:9]) + " > 0", FIX, 1), (" + ".join(n for n, _ in cols[8:]) + " > 0", FIX, 1)], cols, [])
    assert e.value.code == ERR_UNSUPPORTED and "more than 16 referenced columns" in str(e.value)


def test_rule_set_refusals():
    ok = "a > 1"
    for rules, code, word in [([], ERR_INVALID, "no classes"), ([(ok, ACC, 5), (ok, ACC, 4)], ERR_INVALID, "panics"),
                              ([(ok, 2, 5)], ERR_INVALID, "type 2"), ([(ok, FIX, 1)] * 9, ERR_UNSUPPORTED, "9 classes")]:
        with pytest.raises(PgError) as e:
            pa.classcut_compile(rules, COLS, RECALLS)
        assert e.value.code == code and word in str(e.value), str(e.value)
    # decreasing accumulator counts that are not adjacent are the reference's to run
    cc = pa.classcut_compile([(ok, ACC, 5), (ok, FIX, 1), (ok, ACC, 4), (ok, ACC, 4)], COLS, RECALLS)
    for cap, code in ((0, ERR_UNSUPPORTED), (ref.MAX_CAP + 1, ERR_UNSUPPORTED)):
        with pytest.raises(PgError) as e:
            cc.out_cap(cap)
        assert e.value.code == code
    with pytest.raises(PgError) as e:
        pa.candidates_classcut_host(cc, np.zeros((1, 4), np.uint64), np.zeros((1, 4)))
    assert e.value.code == ERR_INVALID and '"a"' in str(e.value)           # the column's values are missing
    cc.free()
    with pytest.raises(PgError) as e:
        pa.classcut_compile([(ok, FIX, 1)], COLS + [("a", pa.F_I64)], RECALLS)
    assert e.value.code == ERR_INVALID and "twice" in str(e.value)
    with pytest.raises(PgError) as e:
        pa.classcut_compile([(ok, FIX, 1)], COLS, ["r%d" % i for i in range(33)])
    assert e.value.code == ERR_UNSUPPORTED and "33 recall names" in str(e.value)


def test_out_cap_is_the_bound():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 9))
        rules, last = [], None
        for _ in range(n):
            ty = int(rng.integers(0, 2))
            cnt = int(rng.integers(0, 40))
            if ty == ACC and last is not None:
                cnt = max(cnt, last)
            last = cnt if ty == ACC else None
            rules.append((ty, cnt))
        cc = pa.classcut_compile([("a > 1", ty, cnt) for ty, cnt in rules], COLS, RECALLS)
        for cap in (1, 7, 50, 300, ref.MAX_CAP):
            assert pa.classcut_out_cap(cc, cap) == ref.out_cap(rules, cap)
        cc.free()
    cc = pa.classcut_compile([("a > 1", FIX, 2**32 - 1), ("a > 1", FIX, 2**32 - 1), ("a > 1", ACC, 2**32 - 1)], COLS, RECALLS)
    assert cc.out_cap(ref.MAX_CAP) == ref.MAX_CAP
    cc.free()


# ---- the whole answer ---------------------------------------------------------------------------------------------------------

def random_case(rng, nq, cap, n_classes=None, optional=(True, True, True, True, True), overlap=0.5):
    """a request batch whose class membership is a column per class: mK > 0; returns everything both sides need"""
    n_classes = n_classes or int(rng.integers(1, ref.MAX_CLASSES + 1))
    rows = rng.permutation(nq * cap * 2)[:nq * cap].astype(np.uint64).reshape(nq, cap)
    rows[rng.random((nq, cap)) < 0.07] = ref.PAD_ROW                             # padding anywhere
    score = rng.integers(0, max(2, cap // 3), (nq, cap)).astype(np.float64)      # many ties
    sp = rng.random((nq, cap)) < 0.05
    score[sp] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0]), int(sp.sum()))
    count = rng.integers(0, cap + 1, nq).astype(np.uint32) if optional[1] else None
    if count is not None and nq > 1:
        count[0], count[-1] = 0, cap
    source = rng.integers(0, 4, (nq, cap)).astype(np.uint8) if optional[0] else None
    p64 = rng.standard_normal((2, nq, cap)) if optional[2] else None
    if p64 is not None:
        p64[rng.random(p64.shape) < 0.05] = np.nan
    smask = rng.integers(0, 16, (nq, cap)).astype(np.uint32) if optional[3] else None
    p32 = rng.standard_normal((3, nq, cap)).astype(np.float32) if optional[4] else None
    member = (rng.random((n_classes, nq, cap)) < overlap)
    cols = {"m%d" % c: member[c].astype(np.int32) for c in range(n_classes)}
    rules, last = [], None
    for c in range(n_classes):
        ty = int(rng.integers(0, 2))
        cnt = int(rng.integers(0, max(2, cap // 2)))
        if ty == ACC and last is not None:
            cnt = max(cnt, last)
        last = cnt if ty == ACC else None
        rules.append((ty, cnt))
    mask = np.zeros((nq, cap), np.uint8)
    for c in range(n_classes):
        mask |= (member[c].astype(np.uint8) << c)
    return dict(rows=rows, score=score, source=source, count=count, planes_f64=p64, source_mask=smask, planes_f32=p32, cols=cols, rules=rules, mask=mask)


def run_host(case, item_in=None):
    decl = [(k, pa.F_I32) for k in case["cols"]]
    cc = pa.classcut_compile([("m%d > 0" % c, ty, cnt) for c, (ty, cnt) in enumerate(case["rules"])], decl, RECALLS)
    try:
        return pa.candidates_classcut_host(cc, case["rows"], case["score"], case["source"], case["count"], case["planes_f64"], case["source_mask"],
                                           case["planes_f32"], case["cols"], item_in)
    finally:
        cc.free()


def want_of(case, mask=None):
    return ref.classcut(case["rules"], case["rows"], case["score"], case["mask"] if mask is None else mask, case["source"], case["count"],
                        case["planes_f64"], case["source_mask"], case["planes_f32"])


def assert_same(got, want, what=""):
    for j, (g, w) in enumerate(zip(got, want)):
        assert ref.same_bits(g, w), (what, j)


def test_restatement_equals_the_go_loop():
    rng = np.random.default_rng(99)
    for i in range(400):
        case = random_case(rng, 1, int(rng.integers(1, 60)), overlap=float(rng.choice([0.2, 0.6, 1.0])))
        cnt = None if case["count"] is None else case["count"][0]
        a = ref.cut_positions(case["rules"], case["rows"][0], case["score"][0], cnt, case["mask"][0])
        b = ref.cut_positions_go(case["rules"], case["rows"][0], case["score"][0], cnt, case["mask"][0])
        assert a == b, i
        assert len(a) <= ref.out_cap(case["rules"], case["rows"].shape[1])


def test_host_statement_equals_the_reference_on_random_cases():
    rng = np.random.default_rng(1234)
    for i in range(60):
        case = random_case(rng, int(rng.integers(1, 5)), int(rng.integers(1, 130)), overlap=float(rng.choice([0.2, 0.6, 1.0])))
        assert_same(run_host(case), want_of(case), i)


OPTIONAL = [(False,) * 5] + [tuple(j == k for j in range(5)) for k in range(5)]


@pytest.mark.parametrize("optional", OPTIONAL, ids=["none", "source", "count", "planes_f64", "source_mask", "planes_f32"])
def test_host_statement_optional_arrays(optional):
    case = random_case(np.random.default_rng(3), 3, 40, optional=optional)
    got = run_host(case)
    assert_same(got, want_of(case))
    assert [g is None for g in got[2:6]] == [not optional[0], not optional[2], not optional[3], not optional[4]]


def edge_case(rules, member_rows, cap=12, score=None):
    """one request of `cap` real entries; member_rows[c]: the positions that are members of class c"""
    case = random_case(np.random.default_rng(0), 1, cap, n_classes=len(rules))
    case["rows"] = np.arange(cap, dtype=np.uint64).reshape(1, cap)
    case["score"] = (np.arange(cap, 0, -1, dtype=np.float64) if score is None else np.asarray(score, np.float64)).reshape(1, cap)
    case["count"] = np.array([cap], np.uint32)
    case["rules"] = rules
    mask = np.zeros((1, cap), np.uint8)
    for c, pos in enumerate(member_rows):
        case["cols"]["m%d" % c] = np.zeros((1, cap), np.int32)
        for p in pos:
            case["cols"]["m%d" % c][0, p] = 1
            mask[0, p] |= 1 << c
    case["mask"] = mask
    return case


def test_host_statement_edges():
    every = list(range(12))
    # a count of 0
    case = edge_case([(FIX, 0), (FIX, 3)], [every, every])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0, :3].tolist() == [0, 1, 2] and got[6][0] == 3
    # a limit of 0 reached through the accumulator: the second class gets nothing although it has fresh members
    case = edge_case([(ACC, 4), (ACC, 4)], [[0, 1, 2, 3, 4], [6, 7, 8]])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0, :got[6][0]].tolist() == [0, 1, 2, 3]
    # a window full of already-taken members: the places are used up, nothing is picked, fresh members lie behind the window
    case = edge_case([(FIX, 3), (FIX, 3)], [[0, 1, 2], [0, 1, 2, 5, 6]])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0, :got[6][0]].tolist() == [0, 1, 2]
    # the accumulator counts picks, not places: class 1 took 2 of its 3 places, class 2 may take 5 - 2 - ... places
    case = edge_case([(FIX, 1), (ACC, 3), (ACC, 5)], [[0], [0, 1, 2, 9], [3, 4, 5, 6, 7]])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0, :got[6][0]].tolist() == [0, 1, 2, 3, 4, 5]
    # a class with no members; all candidates in every class
    case = edge_case([(FIX, 2), (FIX, 2), (ACC, 3)], [[], every, every])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0, :got[6][0]].tolist() == [0, 1, 2]       # the accumulator's window [0, 1, 2] holds one fresh entry
    case = edge_case([(FIX, 2), (FIX, 2), (ACC, 3)], [every, every, every])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0, :got[6][0]].tolist() == [0, 1, 2]
    # d_count of 0: nothing but padding
    case = edge_case([(FIX, 4)], [every])
    case["count"] = np.array([0], np.uint32)
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[6][0] == 0 and (got[0] == ref.PAD_ROW).all() and np.isneginf(got[1]).all() and (got[2] == 0xFF).all()
    # every count 0: out_cap 0
    case = edge_case([(FIX, 0), (ACC, 0)], [every, every])
    got = run_host(case)
    assert got[0].shape == (1, 0) and got[6][0] == 0
    # equal scores keep input position; -0.0 equals +0.0; NaN last
    case = edge_case([(FIX, 12)], [every], score=[1, np.nan, 1, -0.0, 0.0, np.inf, -np.inf, 1, np.nan, 0.0, -0.0, 2])
    got = run_host(case)
    assert_same(got, want_of(case))
    assert got[0][0].tolist() == [5, 11, 0, 2, 7, 3, 4, 9, 10, 6, 1, 8]


def test_host_statement_reads_item_in_and_recall_names():
    rng = np.random.default_rng(11)
    nq, cap = 2, 50
    case = random_case(rng, nq, cap, n_classes=3)
    item_in = (rng.random((nq, cap)) < 0.7).astype(np.uint8)
    trees = [("and", ("cmp", ">", col("m0"), num(0)), ("rn_ne", "hot")), ("or", ("cmp", ">", col("m1"), num(0)), ("rn_eq", "u2i")),
             ("cmp", ">=", ("score",), num(3))]
    rules = [(FIX, 6), (ACC, 9), (ACC, 14)]
    case["rules"] = rules
    mask = np.stack([ref.masks(trees, cap, {k: v[q] for k, v in case["cols"].items()}, item_in[q], case["score"][q], case["source"][q], RECALLS)
                     for q in range(nq)])
    decl = [(k, pa.F_I32) for k in case["cols"]]
    cc = pa.classcut_compile([(ref.render(t), ty, cnt) for t, (ty, cnt) in zip(trees, rules)], decl, RECALLS)
    got = pa.candidates_classcut_host(cc, case["rows"], case["score"], case["source"], case["count"], case["planes_f64"], case["source_mask"],
                                      case["planes_f32"], case["cols"], item_in)
    cc.free()
    assert_same(got, want_of(case, mask))


# ---- the host mirror's config -------------------------------------------------------------------------------------------------------

MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"feed": {"default": {"RecallNames": ["u2i", "hot"]}}},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": 2000, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
        "Recalls": [{"Name": n, "Kind": "vector", "RecallCount": 50, "RecallAlgo": "gpu_faiss", "ItemType": "video"} for n in ("u2i", "hot")],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "classes", "FilterType": "DiversityAdjustCountFilter",
                     "AdjustCountConfs": [{"Expression": "recall_name == 'u2i' && category == 3", "Count": 10, "Type": "fix"},
                                          {"Expression": "[recall_score] > 0.5 || !(brand in (1, 2))", "Count": 20, "Type": "accumulator"},
                                          {"Expression": "recall_name in ('u2i', \"hot\")", "Count": 40, "Type": "accumulator"}]}],
        "FilterNames": {"feed": ["classes"]}}},
}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_parse_recconf.restype = C.c_char_p
    L.ph_parse_recconf.argtypes = [C.c_char_p]
    return L


def test_mirror_config_accepts_the_reference_shape(H):
    assert H.ph_parse_recconf(json.dumps(MIRROR_CONFIG).encode()), H.ph_last_error()


@pytest.mark.parametrize("edit,words", [
    (lambda f: f[0].update({"AdjustCountConfs": []}), (b"pairec_gpu.Filters", b"classes", b"DiversityAdjustCountFilter", b"no classes")),
    (lambda f: f[0].pop("AdjustCountConfs"), (b"pairec_gpu.Filters", b"classes", b"DiversityAdjustCountFilter", b"no classes")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Count": -1}), (b"pairec_gpu.Filters", b"classes", b"Count", b"not a count")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Count": 2.5}), (b"pairec_gpu.Filters", b"classes", b"Count", b"not a count")),
    (lambda f: f[0]["AdjustCountConfs"][1].update({"Type": "weight"}), (b"pairec_gpu.Filters", b"classes", b'Type "weight"')),
    (lambda f: f[0]["AdjustCountConfs"][2].update({"Count": 19}), (b"pairec_gpu.Filters", b"classes", b"DiversityAdjustCountFilter", b"panics")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Expression": "category == 3 ? 1 : 2"}), (b"pairec_gpu.Filters", b"classes", b"ternary")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Expression": "category + 1"}), (b"pairec_gpu.Filters", b"classes", b"is a number, not a bool")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Expression": "title == 'abc'"}), (b"pairec_gpu.Filters", b"classes", b"string literal")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Expression": "category in (3)"}), (b"pairec_gpu.Filters", b"classes", b"one-element")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Expression": "item.category == 3"}), (b"pairec_gpu.Filters", b"classes", b"accessor")),
    (lambda f: f[0].update({"AdjustCountConfs": [{"Expression": "category == 3", "Count": 1, "Type": "fix"}] * 9}),
     (b"pairec_gpu.Filters", b"classes", b"9 classes")),
    (lambda f: f[0].update({"FilterType": "GroupWeightCountFilter"}),
     (b"pairec_gpu.Filters", b'unknown FilterType "GroupWeightCountFilter" (the device serves ItemStateFilter)')),
])
def test_mirror_config_refusals_by_name(H, edit, words):
    cfg = copy.deepcopy(MIRROR_CONFIG)
    edit(cfg["UserDefineConfs"]["pairec_gpu"]["Filters"])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), H.ph_last_error()
