"""CPU tests of the value cap and of DistinctIdSort (csrc/dimcap.hip, csrc/cond.hip): tests/dimcap_ref.py's two
statements of each answer — the array form and the transcription of the Go loops — against each other and against the library's
host statements pg_candidates_dimcap_host / pg_distinct_ids_host, on randomised and constructed lists; the three scenarios of
sort/distinct_id_sort_test.go; every refusal that needs no device, by code and message; the mirror's config refusals; the header's
constants against the ones the kernel is built with."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import cond_ref
import dimcap_ref as ref
import pairec_amd as pa
import trim_ref
from pairec_amd import _lib
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
U32MAX = 0xFFFFFFFF
I64MIN = -(1 << 63)
LIMITS = (1, 2, 3, U32MAX)
MODES = (pa.DIMCAP_NULL_KEEP, pa.DIMCAP_NULL_VALUE)


def random_case(rng, nq, cap, n_values, optional=True):
    keys = rng.integers(0, n_values, (nq, cap)).astype(np.int64)
    keys[rng.random((nq, cap)) < 0.1] = -7                                # the value that may stand for null
    item_in = (rng.random((nq, cap)) > 0.15).astype(np.uint8)
    rows = rng.integers(0, 1 << 40, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < 0.05] = U64MAX                          # padding in the middle of a list
    count = rng.integers(0, cap + 3, nq).astype(np.uint32)               # 0, short of cap, over cap
    score = np.round(rng.standard_normal((nq, cap)), 4)
    score.view(np.uint64)[0, cap // 2] = 0x7FF8000000000123              # a NaN with a payload travels as bits
    if not optional:
        return keys, item_in, (rows, score, None, count, None, None, None)
    return keys, item_in, (rows, score, rng.integers(0, 8, (nq, cap)).astype(np.uint8), count, rng.standard_normal((2, nq, cap)),
                           rng.integers(0, 256, (nq, cap)).astype(np.uint32), rng.standard_normal((3, nq, cap)).astype(np.float32))


def host(keys, item_in, limit, mode, null_value, lists):
    return pa.candidates_dimcap_host((None, limit, mode, null_value), keys, lists[0], lists[1], item_in, *lists[2:])


# ---- the value cap: two statements and the host function -------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("limit", LIMITS)
def test_two_statements_and_the_host_function_agree_on_random_lists(limit, mode):
    rng = np.random.default_rng(1000 * mode + limit % 1000)
    for nq, cap, n_values, optional in ((3, 1, 1, True), (4, 37, 5, True), (2, 300, 40, False), (5, 130, 400, True), (1, 2100, 3, False)):
        keys, item_in, lists = random_case(rng, nq, cap, n_values, optional)
        for null_value in (None, -7):
            a = ref.keep_array(keys, item_in, lists[0], lists[3], limit, mode, null_value)
            g = ref.keep_go(keys, item_in, lists[0], lists[3], limit, mode, null_value)
            assert np.array_equal(a, g), (nq, cap, null_value)
            want = ref.compact(a, *lists)
            trim_ref.same(host(keys, item_in, limit, mode, null_value, lists), want)
            trim_ref.same(host(keys, None, limit, mode, null_value, lists), ref.dimcap(keys, None, limit, mode, null_value, *lists))


def constructed(cap=2100):
    """(name, keys [1][cap], item_in | None, null_value | None): the patterns the kernel's tests use, at a size the Go loops walk"""
    ar = np.arange(cap, dtype=np.int64)
    out = [("distinct", ar + 5, None, None), ("equal", np.full(cap, 9, np.int64), None, None),
           ("all_null", np.full(cap, 4, np.int64), np.zeros(cap, np.uint8), None), ("all_null_value", np.full(cap, 4, np.int64), None, 4),
           ("high_bits", (ar % 7) << 32 | 5, None, None), ("negative", -(ar % 11) - 1, None, None),
           ("int64_min", np.where(ar % 3 == 0, I64MIN, np.where(ar % 3 == 1, I64MIN + 1, -1)).astype(np.int64), None, None),
           ("real_null_value", ar % 5, None, 3), ("real_null_value_unset", ar % 5, None, None)]
    k = ar + 100
    k[1023], k[1024] = 77, 77
    out.append(("chunk_boundary", k, None, None))
    k = ar + 100
    k[960:1024] = 55
    out.append(("one_wave", k, None, None))
    return [(n, np.ascontiguousarray(k)[None, :], None if i is None else i[None, :], nv) for n, k, i, nv in out]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("limit", LIMITS)
def test_constructed_lists(limit, mode):
    rng = np.random.default_rng(5)
    for name, keys, item_in, null_value in constructed():
        cap = keys.shape[1]
        rows = rng.integers(0, 1 << 40, (1, cap)).astype(np.uint64)
        lists = (rows, rng.standard_normal((1, cap)), None, None, None, None, None)
        a = ref.keep_array(keys, item_in, rows, None, limit, mode, null_value)
        assert np.array_equal(a, ref.keep_go(keys, item_in, rows, None, limit, mode, null_value)), name
        got = host(keys, item_in, limit, mode, null_value, lists)
        trim_ref.same(got, ref.compact(a, *lists))
        n = int(got[6][0])
        if name == "distinct":
            assert n == cap
        elif name == "equal":
            assert n == min(limit, cap)
        elif name in ("all_null", "all_null_value"):
            assert n == (cap if mode == pa.DIMCAP_NULL_KEEP else min(limit, cap))
        elif name == "chunk_boundary":
            assert n == (cap - 1 if limit == 1 else cap)
        elif name == "one_wave":
            assert n == cap - 64 + min(limit, 64)
        elif name == "high_bits":
            assert n == min(7 * limit, cap)                           # keys that agree in their low 32 bits are 7 values
        elif name == "int64_min":
            assert n == min(3 * limit, cap)


def test_unique_filter_is_limit_one_and_idempotent():
    rng = np.random.default_rng(3)
    keys, item_in, lists = random_case(rng, 3, 200, 30)
    once = host(keys, item_in, 1, pa.DIMCAP_NULL_KEEP, -7, lists)
    # the kept entries' own keys, carried along as a plane, are the keys of the second pass
    p64 = np.stack([keys.astype(np.float64), item_in.astype(np.float64)])
    first = host(keys, item_in, 1, pa.DIMCAP_NULL_KEEP, -7, (lists[0], lists[1], lists[2], lists[3], p64, lists[5], lists[6]))
    k2, in2 = np.nan_to_num(first[3][0]).astype(np.int64), np.nan_to_num(first[3][1]).astype(np.uint8)
    again = host(k2, in2, 1, pa.DIMCAP_NULL_KEEP, -7, (first[0], first[1], first[2], first[6], first[3], first[4], first[5]))
    trim_ref.same(again, first)
    assert np.array_equal(once[0], first[0])
    for q in range(3):
        n = int(first[6][q])
        real = k2[q, :n][(in2[q, :n] != 0) & (k2[q, :n] != -7)]
        assert real.size == np.unique(real).size


def test_two_dimensions_are_two_calls_in_order():
    rng = np.random.default_rng(4)
    cap = 400
    author, spu = rng.integers(0, 40, (1, cap)).astype(np.int64), rng.integers(0, 15, (1, cap)).astype(np.int64)
    rows = np.arange(cap, dtype=np.uint64)[None, :]
    score = rng.standard_normal((1, cap))
    items = [{"pos": p, "properties": {"author": int(author[0, p]), "spu": int(spu[0, p])}} for p in range(cap)]
    for order in (("author", 2, "spu", 5), ("spu", 5, "author", 2)):
        want = ref.go_group_weight_dimension(ref.go_group_weight_dimension(items, order[0], order[1]), order[2], order[3])
        col = {"author": author, "spu": spu}
        one = pa.candidates_dimcap_host((None, order[1], pa.DIMCAP_NULL_VALUE, None), col[order[0]], rows, score)
        n = int(one[6][0])
        k2 = np.zeros((1, cap), np.int64)
        k2[0, :n] = col[order[2]][0, one[0][0, :n].astype(np.int64)]
        two = pa.candidates_dimcap_host((None, order[3], pa.DIMCAP_NULL_VALUE, None), k2, one[0], one[1], count=one[6])
        assert two[0][0, :int(two[6][0])].tolist() == [it["pos"] for it in want]


# ---- DistinctIdSort ---------------------------------------------------------------------------------------------------------------

STR = {"r1": 1, "r2": 2}
COLS = [("recall_name", pa.F_I64)]


def go_items():
    """distinct_id_sort_test.go: 20 items, recall r1 for the first ten and r2 for the rest"""
    return [{"id": str(i), "score": float(i), "properties": {"recall_name": "r1" if i < 10 else "r2"}} for i in range(20)]


def equal_rule(value):
    return [{"Name": "recall_name", "Operator": "equal", "Domain": "item", "Type": "string", "Value": value}]


def lib_ids(rules, ids, items):
    cond = pa.cond_compile([{"Conditions": r} for r in rules], COLS, strings=dict(STR))
    try:
        return pa.distinct_ids_host(cond, ids, {"recall_name": np.array([STR[it["properties"]["recall_name"]] for it in items], np.int64)})
    finally:
        cond.free()


def string_equal(rule, i, item):
    return item["properties"].get(rule[0]["Name"]) == rule[0]["Value"], None


@pytest.mark.parametrize("name", ("__distinct_id__", "__recall_name__"))
def test_go_scenarios_default_and_named(name):
    items = ref.go_distinct_id_sort(go_items(), [(equal_rule("r1"), -1, name)], string_equal)
    want = [-1] * 10 + [i + 1 for i in range(10, 20)]
    assert [it["properties"][name] for it in items] == want
    assert lib_ids([equal_rule("r1")], [-1], items).tolist() == want
    match = np.array([[it["properties"]["recall_name"] == "r1" for it in items]])
    assert ref.distinct_ids_array(match, [-1]).tolist() == want


def test_go_scenario_two_sorts_in_sequence():
    items = go_items()
    ref.go_distinct_id_sort(items, [(equal_rule("r1"), -1, "__recall_name1__")], string_equal)
    ref.go_distinct_id_sort(items, [(equal_rule("r2"), -1, "__recall_name2__")], string_equal)
    want1 = [-1] * 10 + [i + 1 for i in range(10, 20)]
    want2 = [i + 1 for i in range(10)] + [-1] * 10
    assert [it["properties"]["__recall_name1__"] for it in items] == want1
    assert [it["properties"]["__recall_name2__"] for it in items] == want2
    assert lib_ids([equal_rule("r1")], [-1], items).tolist() == want1
    assert lib_ids([equal_rule("r2")], [-1], items).tolist() == want2


RULES8 = [
    [{"Name": "a", "Operator": "equal", "Type": "int", "Value": 3}],
    [{"Name": "b", "Operator": "greater", "Type": "float", "Value": 0.5}, {"Name": "ui", "Domain": "user", "Operator": "equal", "Type": "int", "Value": 7}],
    [{"Name": "a", "Operator": "in", "Type": "int", "Value": [1, 2, 9]}],
    [{"Name": "c", "Operator": "not_equal", "Type": "int64", "Value": "item.a"}, {"Name": "b", "Operator": "less", "Type": "float", "Value": -0.5}],
    [{"Name": "uf", "Domain": "user", "Operator": "is_not_null"}, {"Name": "a", "Operator": "equal", "Type": "int", "Value": 5}],
    [{"Operator": "bool", "Type": "or", "Configs": [{"Name": "a", "Operator": "equal", "Type": "int", "Value": 6},
                                                     {"Name": "c", "Operator": "equal", "Type": "int64", "Value": 1 << 40}]}],
    [{"Name": "a", "Operator": "is_null"}],
    [{"Name": "b", "Operator": "lessThan", "Type": "float", "Value": "user.uf"}],
]
IDS8 = [-1, 1 << 33, 5, -(1 << 40), 0, 2147483648, 77, -2]
DECL8 = [("a", pa.F_I32), ("b", pa.F_F64), ("c", pa.F_I64)]


def test_distinct_ids_two_statements_and_the_host_function_on_eight_rules():
    rng = np.random.default_rng(8)
    n = 500
    cols = {"a": rng.integers(0, 12, n).astype(np.int32), "b": rng.standard_normal(n),
            "c": rng.choice([0, 3, 1 << 40], n).astype(np.int64)}
    inside = rng.random(n) > 0.2
    cond = pa.cond_compile([{"Conditions": r} for r in RULES8], DECL8)
    try:
        seen = set()
        for user in ({"ui": 7, "uf": 0.25}, {"ui": 8}, {}):
            match = np.array([[cond_ref.match(r, i, cols, inside, user) for i in range(n)] for r in RULES8])
            want = ref.distinct_ids_array(match, IDS8)
            items = [{"properties": {}} for _ in range(n)]
            ref.go_distinct_id_sort(items, [(r, IDS8[k], "d") for k, r in enumerate(RULES8)],
                                    lambda rule, i, item: (cond_ref.match(rule, i, cols, inside, user), None))
            assert [it["properties"]["d"] for it in items] == want.tolist()
            got = pa.distinct_ids_host(cond, IDS8, cols, inside, user)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            seen |= set(want.tolist())
        assert set(IDS8) <= seen and any(0 < v <= n and v not in IDS8 for v in seen)       # every rule is some item's first; some match none
    finally:
        cond.free()


def test_an_evaluation_error_is_a_non_match():
    """distinct_id_sort.go:60: err != nil falls to the else branch, as a false flag does"""
    def evaluate(rule, i, item):
        return True, ("boom" if i % 2 else None)
    items = ref.go_distinct_id_sort([{"properties": {}} for _ in range(6)], [("r", 9, "d")], evaluate)
    assert [it["properties"]["d"] for it in items] == [9, 2, 9, 4, 9, 6]


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------

def raises(code, text, fn, *args):
    with pytest.raises(PgError) as ei:
        fn(*args)
    assert ei.value.code == code and str(ei.value).endswith(text), str(ei.value)


def test_dimcap_host_refusals_by_code_and_message():
    L = _lib.load()
    d = 1 << 20                                                          # made-up addresses: every call is refused before it reads one
    who = "pg_candidates_dimcap_host: "

    def call(conf=(None, 1, 0, None), nq=1, cap=16, **kw):
        a = dict(keys=9 * d, item_in=0, rows=d, score=2 * d, source=3 * d, count=0, planes_f64=0, n_f64=0, source_mask=0, planes_f32=0, n_f32=0,
                 out_rows=4 * d, out_score=5 * d, out_source=6 * d, out_planes_f64=0, out_source_mask=0, out_planes_f32=0, out_count=7 * d)
        a.update(kw)
        c = None if conf is None else C.byref(pa.engine._dimcap_conf(conf))
        _lib.check(L.pg_candidates_dimcap_host(c, nq, cap, *[a[k] or None if k not in ("n_f64", "n_f32") else a[k] for k in a]))

    for kw, code, text in ((dict(conf=None), -1, "NULL argument"), (dict(keys=0), -1, "NULL argument"), (dict(rows=0), -1, "NULL argument"),
                           (dict(out_count=0), -1, "NULL argument"),
                           (dict(conf=(None, 0, 0, None)), -1, "limit=0 keeps nothing (1 .. UINT32_MAX; 1 is DimensionFieldUniqueFilter)"),
                           (dict(conf=(None, 1, 2, None)), -1, "unknown null_mode 2"),
                           (dict(nq=0), -1, "nq=0 must be in [1,256]"), (dict(nq=257), -1, "nq=257 must be in [1,256]"),
                           (dict(cap=0), -4, "cap=0 unsupported (1..16384)"), (dict(cap=16385), -4, "cap=16385 unsupported (1..16384)"),
                           (dict(out_source=0), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(source_mask=8 * d), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(planes_f64=8 * d, n_f64=1), -1, "a carried plane set and its output come in pairs"),
                           (dict(planes_f32=8 * d, out_planes_f32=10 * d, n_f32=9), -1, "a carried plane set holds 1..8 planes"),
                           (dict(planes_f64=8 * d, out_planes_f64=10 * d, n_f64=0), -1, "a carried plane set holds 1..8 planes"),
                           (dict(out_rows=d + 64), -1, "an output overlaps its input"),
                           (dict(out_score=2 * d - 8), -1, "an output overlaps its input")):
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code == code and str(ei.value).endswith(who + text), (kw, str(ei.value))
    # the order of the checks: the conf before nq, nq before cap, cap before the pairing, the pairing before the overlap
    for kw, text in ((dict(conf=(None, 0, 0, None), nq=0), "limit=0"), (dict(nq=0, cap=0), "nq=0"), (dict(cap=0, out_source=0), "cap=0"),
                     (dict(out_source=0, out_rows=d), "come in pairs")):
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert text in str(ei.value), (kw, str(ei.value))


def test_device_entries_without_a_context():
    L = _lib.load()
    d = 1 << 20
    conf = pa.engine._dimcap_conf(("author", 1, 0, None))
    v = lambda p: C.c_void_p(p or None)                                              # noqa: E731
    raises(-1, "pg_candidates_dimcap_dev: NULL argument", lambda: _lib.check(L.pg_candidates_dimcap_dev(
        None, v(d), C.byref(conf), 1, 16, v(d), v(d), None, None, None, 0, None, None, 0, v(d), v(d), None, None, None, None, v(d))))
    raises(-1, "pg_candidates_dimcap: NULL argument", lambda: _lib.check(L.pg_candidates_dimcap(
        None, v(d), C.byref(conf), 16, v(d), v(d), None, v(d), v(d), None, v(d))))
    ids = np.array([1], np.int64)
    raises(-1, "pg_distinct_ids_dev: NULL argument", lambda: _lib.check(L.pg_distinct_ids_dev(
        None, v(d), v(d), ids.ctypes.data_as(C.c_void_p), 1, 16, v(d), None, None, None, v(d))))
    raises(-1, "pg_distinct_ids: NULL argument", lambda: _lib.check(L.pg_distinct_ids(
        None, v(d), ids.ctypes.data_as(C.c_void_p), 16, None, None, None, 0, v(d))))


def test_distinct_ids_host_refusals():
    L = _lib.load()
    cond = pa.cond_compile([{"Conditions": r} for r in RULES8[:2]], DECL8)
    boost = pa.cond_compile([{"Conditions": [], "Expression": "score + 1"}], DECL8, boost=True)
    try:
        with pytest.raises(ValueError, match="1 ids for 2 rules"):
            pa.distinct_ids_host(cond, [1], {"a": np.zeros(3, np.int32), "b": np.zeros(3)})
        raises(-1, "pg_distinct_ids_host: the set was compiled as a boost rule set", pa.distinct_ids_host, boost, [1], None, None, None, 3)
        raises(-1, 'pg_distinct_ids_host: the values of column "b" are missing', pa.distinct_ids_host, cond, [1, 2], {"a": np.zeros(3, np.int32)})
        out = np.zeros(3, np.int64)
        raises(-1, "pg_distinct_ids_host: NULL argument", lambda: _lib.check(L.pg_distinct_ids_host(cond.h, None, 3, None, None, None, 0, out.ctypes.data_as(C.c_void_p))))
        cols = (C.c_void_p * 3)(np.zeros(3, np.int32).ctypes.data, np.zeros(3).ctypes.data, None)
        ids = np.array([1, 2], np.int64)
        raises(-1, 'pg_distinct_ids_host: the set reads user property "ui" but user_vals is NULL', lambda: _lib.check(L.pg_distinct_ids_host(
            cond.h, ids.ctypes.data_as(C.c_void_p), 3, None, cols, None, 0, out.ctypes.data_as(C.c_void_p))))
        assert pa.distinct_ids_host(cond, [1, 2], None, None, None, 0).size == 0         # an empty request: an empty answer
    finally:
        cond.free()
        boost.free()


# ---- the mirror's config ------------------------------------------------------------------------------------------------------------

MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SortConfs": [{"Name": "host_side", "SortType": "DistinctIdSort"}],                 # declared there it stays skipped
    "SceneConfs": {"feed": {"default": {"RecallNames": ["u2i"]}}},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": 2000, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
        "Recalls": [{"Name": "u2i", "Kind": "vector", "RecallCount": 50, "RecallAlgo": "gpu_faiss", "ItemType": "video"}],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "one_per_author", "FilterType": "DimensionFieldUniqueFilter", "Dimension": "author", "NullValue": 0,
                     "FeatureStore": "item_features"},
                    {"Name": "one_per_spu", "FilterType": "DimensionFieldUniqueFilter", "Dimension": "spu"}],
        "FilterNames": {"feed": ["one_per_author"]},
        "Sorts": [{"Name": "tag", "SortType": "DistinctIdSort", "DistinctIdConditions": [
            {"DistinctId": -1, "Conditions": equal_rule("r1")},
            {"DistinctId": 5, "DistinctIdName": "__distinct_id__", "Conditions": [{"Name": "level", "Operator": "greater", "Type": "int", "Value": 3}]}]}]}},
}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_parse_recconf.restype = C.c_char_p
    L.ph_parse_recconf.argtypes = [C.c_char_p]
    return L


def test_mirror_config_accepts_the_filter_and_the_sort(H):
    assert H.ph_parse_recconf(json.dumps(MIRROR_CONFIG).encode()), H.ph_last_error()


@pytest.mark.parametrize("edit,words", [
    (lambda g: g["Filters"][0].update({"Dimension": ""}), (b"pairec_gpu.Filters", b"one_per_author", b"DimensionFieldUniqueFilter", b"Dimension is empty")),
    (lambda g: g["Filters"][1].pop("Dimension"), (b"pairec_gpu.Filters", b"one_per_spu", b"DimensionFieldUniqueFilter", b"Dimension is empty")),
    (lambda g: g["Filters"][0].update({"NullValue": "x"}), (b"pairec_gpu.Filters", b"one_per_author", b"NullValue is not an integer")),
    (lambda g: g["Filters"][0].update({"NullValue": 1.5}), (b"pairec_gpu.Filters", b"one_per_author", b"NullValue is not an integer")),
    (lambda g: g["Filters"][0].update({"FeatureStore": "elsewhere"}), (b"pairec_gpu.Filters", b"one_per_author", b'FeatureStore "elsewhere"')),
    (lambda g: g["Filters"][1].update({"FilterType": "GroupWeightCountFilter"}),
     (b"pairec_gpu.Filters", b'unknown FilterType "GroupWeightCountFilter" (the device serves ItemStateFilter)')),
    (lambda g: g["Sorts"][0]["DistinctIdConditions"][1].update({"DistinctIdName": "__other__"}),
     (b"pairec_gpu.Sorts", b"tag", b"DistinctIdSort", b'"__other__"', b'"__distinct_id__"', b"the device serves one name per sort")),
    (lambda g: g["Sorts"][0]["DistinctIdConditions"][1]["Conditions"][0].update({"Type": "bogus"}),
     (b"pairec_gpu.Sorts", b"tag", b"DistinctIdSort", b'Type "bogus" of "level" is not served')),
    (lambda g: g["Sorts"][0]["DistinctIdConditions"][0].update({"DistinctId": 1.5}), (b"pairec_gpu.Sorts", b"tag", b"DistinctId is not an integer")),
    (lambda g: g["Sorts"][0].update({"DistinctIdConditions": [{"DistinctId": 1, "Conditions": []}] * 9}),
     (b"pairec_gpu.Sorts", b"tag", b"more than 8 DistinctIdConditions")),
])
def test_mirror_config_refusals_by_name(H, edit, words):
    cfg = copy.deepcopy(MIRROR_CONFIG)
    edit(cfg["UserDefineConfs"]["pairec_gpu"])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), (w, H.ph_last_error())


# ---- the constants -------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_kernel_agree_on_the_constants():
    with open(os.path.join(ROOT, "include", "pairec_gpu.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "pairec_amd", "csrc", "dimcap.hip")) as f:
        hip = f.read()
    for name, value in (("PG_DIMCAP_CHUNK", pa.DIMCAP_CHUNK), ("PG_DIMCAP_MIN_SLOTS", pa.DIMCAP_MIN_SLOTS), ("PG_DIMCAP_LDS_MAX_CAP", pa.DIMCAP_LDS_MAX_CAP)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    assert "kDimcapLdsMaxCap = %d" % pa.DIMCAP_LDS_MAX_CAP in hip and "kSlotDimcap" in hip
    assert "PG_DIMCAP_NULL_KEEP = %d, PG_DIMCAP_NULL_VALUE = %d" % (pa.DIMCAP_NULL_KEEP, pa.DIMCAP_NULL_VALUE) in header
    # the table at the boundary fits a workgroup's LDS; one entry more does not keep the load factor
    assert 12 * ref.slots_of(pa.DIMCAP_LDS_MAX_CAP) + 8 + 1024 <= 160 * 1024 < 12 * ref.slots_of(2 * pa.DIMCAP_LDS_MAX_CAP)
    assert ref.first_slot(-1, 2048) < 2048 and len(set(ref.colliding_keys(1024, 5).tolist())) == 5
