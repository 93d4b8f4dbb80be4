"""CPU checks behind DiversityRuleSort on the device: tests/diversity_ref.py — the specification the GPU tests
compare with — against a literal, item-by-item transcription of the reference's loops (sort/diversity_rule_sort.go:116-283,
sort/diversity_rule.go:34-92, sort/diversity_exclusion_rule.go:37-56: maps keyed by item id, items[1:] and all) on the reference's own
test cases (tests/golden/diversity_rule_sort.json) and on random small ones; pg_diversity_rules_host, the host statement of what the
kernel computes, against diversity_ref; every refusal; the header's limits against the ones csrc/diversity.hip is built with; and
the host mirror's config parse."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import diversity_ref as ref
import pairec_amd as pa
from pairec_amd import _lib
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4

with open(os.path.join(ROOT, "tests", "golden", "diversity_rule_sort.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


# ---- the reference's loops, item by item --------------------------------------------------------------------------------------------

class GoRule:
    """DiversityRule (diversity_rule.go:20-97); an item is {"Id", "RetrieveId", "props": {name: string}}"""

    def __init__(self, config):
        self.c, self.DimensionItemMap = config, {}

    def GetDimensionValue(self, item):
        if item["Id"] in self.DimensionItemMap:
            return self.DimensionItemMap[item["Id"]]
        self.DimensionItemMap[item["Id"]] = "_".join(item["props"].get(d, "") for d in self.c["Dimensions"])
        return self.DimensionItemMap[item["Id"]]

    def Match(self, item, itemList):
        size = len(itemList)
        value = self.GetDimensionValue(item)
        if self.c["IntervalSize"] > 0 and size >= self.c["IntervalSize"]:
            end, begin, sameValue = size, size - self.c["IntervalSize"], 1
            i = end - 1
            while i >= begin:
                if value == self.GetDimensionValue(itemList[i]):
                    sameValue += 1
                else:
                    break
                i -= 1
            if sameValue > self.c["IntervalSize"]:
                return False
        if self.c["WindowSize"] > 0 and self.c["FrequencySize"] > 0 and self.c["WindowSize"] > self.c["FrequencySize"]:
            end, begin = size, size - self.c["WindowSize"] + 1
            if begin < 0:
                begin = 0
            sameValue = 1
            for i in range(begin, end):
                if value == self.GetDimensionValue(itemList[i]):
                    sameValue += 1
                if sameValue > self.c["FrequencySize"]:
                    return False
        return True


class GoExclusionRule:
    """DiversityExclusionRule (diversity_exclusion_rule.go:11-56); Conditions: [(name, op, integer)] over the props' integers"""

    def __init__(self, config):
        self.positions = {p: True for p in config["Positions"]}
        self.conditions, self.DimensionItemMap = config["Conditions"], {}

    def Match(self, position, item):
        if position not in self.positions:
            return False
        if not self.conditions:
            return False
        if item["Id"] in self.DimensionItemMap:
            return self.DimensionItemMap[item["Id"]]
        flag = all(ref._OPS[op](int(item["props"][name]), value) for name, op, value in self.conditions)
        self.DimensionItemMap[item["Id"]] = flag
        return flag


def go_do_sort(config, size, items):
    """DiversityRuleSort.doSort (:116-283); returns the new Data"""
    diversityRules = [GoRule(c) for c in config["DiversityRules"]]
    if len(diversityRules) == 0:
        return items
    exclusionRules = [GoExclusionRule(c) for c in config.get("ExclusionRules", [])]
    excludeItems = []
    if len(config.get("ExcludeRecalls", [])) > 0:
        newItems = []
        for item in items:
            if item["RetrieveId"] in config["ExcludeRecalls"]:
                excludeItems.append(item)
            else:
                newItems.append(item)
        original, items = items, newItems
    else:
        original = items
    itemLength = len(items)
    if itemLength == 0:
        return original
    diversitySize = size
    if config.get("DiversitySize", 0) > 0:
        diversitySize = config["DiversitySize"]
        if diversitySize > itemLength:
            diversitySize = itemLength
    explore = config["ExploreItemSize"] if config.get("ExploreItemSize", 0) > 0 else -1
    result, alreadyMatchItems = [], {}
    if len(exclusionRules) > 0:
        for item in items:
            exFlag = False
            for rule in exclusionRules:
                if rule.Match(1, item):
                    exFlag = True
                    break
            if not exFlag:
                alreadyMatchItems[item["Id"]] = True
                result.append(item)
                break
        if len(result) == 0:
            alreadyMatchItems[items[0]["Id"]] = True
            result.append(items[0])
            items = items[1:]
    else:
        alreadyMatchItems[items[0]["Id"]] = True
        result.append(items[0])
        items = items[1:]
    index = 1
    hasWeight = any(r.c.get("Weight", 0) > 0 for r in diversityRules)
    while len(result) <= diversitySize:
        if index == itemLength:
            break
        flag, firstItemIndex = True, -1
        container = {"item": None, "maxWeight": 0}
        for i, item in enumerate(items):
            if item["Id"] in alreadyMatchItems:
                continue
            if len(exclusionRules) > 0:
                exFlag = False
                for rule in exclusionRules:
                    if rule.Match(len(result) + 1, item):
                        exFlag = True
                        break
                if exFlag:
                    continue
            if firstItemIndex == -1:
                firstItemIndex = i
            if explore > 0 and i - firstItemIndex >= explore:
                break
            flag, weight = True, 0
            for rule in diversityRules:
                if hasWeight:
                    if rule.Match(item, result):
                        weight += rule.c.get("Weight", 0)
                    else:
                        flag = False
                else:
                    flag = rule.Match(item, result)
                    if not flag:
                        break
            if flag:
                alreadyMatchItems[item["Id"]] = True
                result.append(item)
                index += 1
                break
            if container["item"] is None:
                container["item"], container["maxWeight"] = item, weight
            elif container["maxWeight"] < weight:
                container["item"], container["maxWeight"] = item, weight
        if not flag:
            item = container["item"] if container["item"] is not None else items[firstItemIndex]
            alreadyMatchItems[item["Id"]] = True
            result.append(item)
            index += 1
        elif firstItemIndex == -1:
            break
    for item in items:
        if item["Id"] in alreadyMatchItems:
            continue
        result.append(item)
    return result + excludeItems


def literal(cfg, n, cols, source=None, enable=True):
    """the dict config and integer columns of diversity_ref.sort_one through the reference's loops"""
    if not enable:
        return list(range(n))
    items = [{"Id": "id%d" % p, "pos": p, "RetrieveId": "r%d" % (int(source[p]) if source is not None else 0),
              "props": {"c%d" % c: str(int(cols[c][p])) for c in range(len(cols))}} for p in range(n)]
    mask = cfg.get("exclude_source_mask", 0)
    config = {"DiversityRules": [{"Dimensions": ["c%d" % c for c in r["dims"]], "IntervalSize": r.get("interval", 0), "WindowSize": r.get("window", 0),
                                  "FrequencySize": r.get("frequency", 0), "Weight": r.get("weight", 0)} for r in cfg.get("rules", [])],
              "ExclusionRules": [{"Positions": list(e["positions"]), "Conditions": [("c%d" % c, op, v) for c, op, v in e["terms"]]}
                                 for e in cfg.get("exclusions", [])],
              "ExcludeRecalls": ["r%d" % s for s in range(32) if (mask >> s) & 1] if source is not None else [],
              "DiversitySize": cfg.get("diversity_size", 0), "ExploreItemSize": cfg.get("explore_item_size", 0)}
    return [it["pos"] for it in go_do_sort(config, cfg.get("size", 0), items)]


def golden_case(case):
    cols = [case["columns"][name] for name in case["column_names"]]
    return case["config"] | {"exclusions": [{"positions": e["positions"], "terms": [tuple(t) for t in e["terms"]]}
                                            for e in case["config"].get("exclusions", [])]}, len(cols[0]), cols


def host(cfg, n, cols, source=None, enable=True):
    dims = np.asarray(cols, dtype=np.int64).reshape(len(cols), 1, -1)[:, :, :n] if n else np.zeros((len(cols), 1, 0), np.int64)
    out = pa.diversity_rules_host(cfg, np.ascontiguousarray(dims), None, None if source is None else np.asarray(source, np.uint8)[None, :n],
                                  None if enable else np.zeros(1, np.uint8))
    return out[0].tolist()


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_cases_reference_loops_spec_and_host_function(case):
    cfg, n, cols = golden_case(case)
    want = case["expected_order"]
    assert literal(cfg, n, cols) == want
    assert ref.sort_one(cfg, n, cols) == want
    assert host(cfg, n, cols) == want
    # what sort/diversity_rule_sort_test.go itself asserts about the case
    for a in case["reference_asserts"]:
        col = cols[case["column_names"].index(a["column"])] if "column" in a else None
        for i in a["result_indices"]:
            if col is not None:
                assert col[want[i]] == a["equals"], (case["name"], i)
            else:
                assert want[i] == a["item"][a["result_indices"].index(i)], (case["name"], i)


def random_case(rng):
    n = int(rng.integers(0, 41))
    n_cols = int(rng.integers(1, 5))
    cols = [rng.integers(0, int(rng.integers(1, 5)), max(n, 1)).tolist() for _ in range(n_cols)]
    rules = []
    for _ in range(int(rng.integers(1, 4))):
        rules.append({"dims": rng.integers(0, n_cols, int(rng.integers(1, 3))).tolist(), "interval": int(rng.integers(0, 4)),
                      "window": int(rng.integers(0, 8)), "frequency": int(rng.integers(0, 4)),
                      "weight": int(rng.choice([0, 0, 0, -3, -1, 1, 2, 5]))})
    if rng.random() < 0.3:
        for r in rules:
            r["weight"] = 0
    excl = []
    for _ in range(int(rng.integers(0, 3))):
        positions = sorted(set(rng.integers(1, 14, int(rng.integers(1, 5))).tolist()))
        if rng.random() < 0.25:                                      # excludes everything at its positions
            terms = [(0, ref.GE, 0)]
        else:
            terms = [(int(rng.integers(0, n_cols)), int(rng.integers(0, 6)), int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 3)))]
        excl.append({"positions": positions, "terms": terms})
    cfg = {"size": int(rng.choice([0, 1, 5, n, n + 7])), "diversity_size": int(rng.choice([0, 0, 3, n + 5])),
           "explore_item_size": int(rng.choice([0, 0, -1, 1, 3, 8])), "rules": rules, "exclusions": excl}
    source = None
    if rng.random() < 0.4:
        source = rng.integers(0, 4, max(n, 1)).astype(np.uint8)
        cfg["exclude_source_mask"] = int(rng.choice([0b0001, 0b0110, 0b1111]))
    return cfg, n, cols, source


def test_spec_and_host_function_read_the_sort_as_its_loops_do():
    rng = np.random.default_rng(20240917)
    fallbacks = 0
    for i in range(3000):
        cfg, n, cols, source = random_case(rng)
        want = literal(cfg, n, cols, source)
        assert sorted(want) == list(range(n))
        assert ref.sort_one(cfg, n, cols, source) == want, (i, cfg, cols, source)
        assert host(cfg, n, cols, source) == want, (i, cfg, cols, source)
        fallbacks += want != list(range(n))
    assert fallbacks > 1000                                          # (the cases are not all identities)


def test_enable_count_and_batches_on_the_host():
    rng = np.random.default_rng(5)
    nq, cap = 7, 33
    dims = rng.integers(0, 3, (2, nq, cap))
    cfg = {"size": 10, "rules": [{"dims": [0], "interval": 1}, {"dims": [0, 1], "window": 4, "frequency": 1, "weight": 2}],
           "exclusions": [{"positions": [1, 3], "terms": [(1, ref.EQ, 0)]}], "exclude_source_mask": 2}
    count = rng.integers(0, cap + 1, nq).astype(np.uint32)
    source = rng.integers(0, 3, (nq, cap)).astype(np.uint8)
    enable = np.array([1, 0, 1, 1, 0, 7, 1], np.uint8)
    want = ref.diversity_rules(cfg, dims, count, source, enable)
    assert np.array_equal(pa.diversity_rules_host(cfg, dims, count, source, enable), want)
    for q in range(nq):
        n = int(count[q])
        assert sorted(want[q, :n].tolist()) == list(range(n)) and (want[q, n:] == ref.NONE).all()
        if not enable[q]:
            assert want[q, :n].tolist() == list(range(n))
    assert np.array_equal(pa.diversity_rules_host({"size": 10}, dims, count), ref.diversity_rules({"size": 10}, dims, count))   # no rules


def test_host_function_at_the_largest_request():
    rng = np.random.default_rng(8192)
    n = ref.MAX_N
    dims = np.stack([rng.integers(0, 6, n), rng.integers(0, 3, n), np.arange(n) // 700]).reshape(3, 1, n)
    cfg = {"size": 60, "explore_item_size": 3000, "rules": [{"dims": [0], "window": 10, "frequency": 2, "weight": 1},
                                                          {"dims": [1, 2], "interval": 2, "weight": 4}, {"dims": [2], "window": 40, "frequency": 3}],
           "exclusions": [{"positions": [1, 2, 30, 61], "terms": [(0, ref.LE, 1)]}]}
    want = ref.diversity_rules(cfg, dims)
    assert np.array_equal(pa.diversity_rules_host(cfg, dims), want) and want[0, :61].tolist() != list(range(61))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

RULE = {"dims": [0], "interval": 1}
EXCL = {"positions": [1], "terms": [(0, ref.EQ, 1)]}


@pytest.mark.parametrize("cfg,kw,code,word", [
    ({"rules": [{"dims": [], "interval": 1}]}, {}, INVALID, "n_dims"),
    ({"rules": [{"dims": [0, 0, 0, 0, 0], "interval": 1}]}, {}, INVALID, "n_dims"),
    ({"rules": [{"dims": [2], "interval": 1}]}, {}, INVALID, "column index 2"),
    ({"rules": [{"dims": [0], "interval": -1}]}, {}, INVALID, "negative"),
    ({"rules": [{"dims": [0], "window": -5, "frequency": 1}]}, {}, INVALID, "negative"),
    ({"rules": [{"dims": [0], "window": 5, "frequency": -1}]}, {}, INVALID, "negative"),
    ({"rules": [RULE], "exclusions": [{"positions": [1], "terms": [(0, 6, 1)]}]}, {}, INVALID, "operator"),
    ({"rules": [RULE], "exclusions": [{"positions": [1], "terms": [(0, -1, 1)]}]}, {}, INVALID, "operator"),
    ({"rules": [RULE], "exclusions": [{"positions": [1], "terms": [(2, ref.EQ, 1)]}]}, {}, INVALID, "column index 2"),
    ({"rules": [RULE], "exclusions": [{"positions": [3, 0], "terms": [(0, ref.EQ, 1)]}]}, {}, INVALID, "position 0"),
    ({"rules": [RULE], "exclusions": [{"positions": [], "terms": [(0, ref.EQ, 1)]}]}, {}, INVALID, "no position"),
    ({"rules": [RULE], "exclusions": [{"positions": [1], "terms": []}]}, {}, INVALID, "no term"),
    ({"rules": [RULE], "exclude_source_mask": 1}, {}, INVALID, "exclude_source_mask"),
    ({"rules": [RULE] * 9}, {}, UNSUPPORTED, "n_rules"),
    ({"rules": [RULE], "exclusions": [EXCL] * 9}, {}, UNSUPPORTED, "n_excl"),
    ({"rules": [RULE], "exclusions": [{"positions": [1], "terms": [(0, ref.EQ, 1)] * 5}]}, {}, UNSUPPORTED, "terms"),
    ({"rules": [RULE], "exclusions": [{"positions": list(range(1, 66)), "terms": [(0, ref.EQ, 1)]}]}, {}, UNSUPPORTED, "positions"),
    ({"rules": [RULE], "multi_value": 1}, {}, UNSUPPORTED, "MultiValueDimensionConf"),
    ({"rules": [RULE]}, {"cap": ref.MAX_N + 1}, UNSUPPORTED, "cap"),
    ({"rules": [RULE]}, {"nq": 257}, UNSUPPORTED, "nq"),
    ({"rules": [RULE]}, {"n_cols": 17}, UNSUPPORTED, "n_cols"),
])
def test_refused_configs(cfg, kw, code, word):
    dims = np.zeros((kw.get("n_cols", 2), kw.get("nq", 1), kw.get("cap", 4)), np.int64)
    with pytest.raises(PgError) as ei:
        pa.diversity_rules_host(cfg, dims)
    assert ei.value.code == code and "pg_diversity_rules_host" in str(ei.value) and word in str(ei.value)


def test_accepted_edges():
    dims = np.zeros((2, 1, 4), np.int64)
    assert pa.diversity_rules_host({}, dims)[0].tolist() == [0, 1, 2, 3]                                  # no rules: the identity
    far = {"rules": [RULE], "size": 4, "exclusions": [{"positions": [1] + list(range(9000, 9100)), "terms": [(0, ref.EQ, 1)]}]}
    assert pa.diversity_rules_host(far, dims)[0].tolist() == [0, 1, 2, 3]                                 # positions nothing reaches do not count
    assert pa.diversity_rules_host({"rules": [RULE], "exclude_source_mask": 1}, dims, source=np.zeros((1, 4), np.uint8))[0].tolist() == [0, 1, 2, 3]
    L = _lib.load()
    assert L.pg_diversity_rules_host(None, 1, 4, None, None, None, None, None) == INVALID
    assert L.pg_diversity_rules_dev(None, None, 1, 4, None, None, None, None, None) == INVALID
    assert L.pg_diversity_rules(None, None, 4, None, None, None) == INVALID
    assert L.pg_diversity_rules_features_dev(None, None, None, None, 1, 4, None, None, None, None, None) == INVALID


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_header_constants_are_the_kernels_and_the_tests():
    with open(os.path.join(ROOT, "include", "pairec_gpu.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "pairec_amd", "csrc", "diversity.hip")) as f:
        hip = f.read()
    for macro, const, mine, engine in (("PG_DIV_MAX_N", "kDivMaxN", ref.MAX_N, pa.DIV_MAX_N), ("PG_DIV_MAX_RULES", "kDivMaxRules", ref.MAX_RULES, pa.DIV_MAX_RULES),
                                       ("PG_DIV_MAX_DIMS", "kDivMaxDims", ref.MAX_DIMS, pa.DIV_MAX_DIMS), ("PG_DIV_MAX_COLS", "kDivMaxCols", ref.MAX_COLS, pa.DIV_MAX_COLS),
                                       ("PG_DIV_MAX_EXCL", "kDivMaxExcl", ref.MAX_EXCL, pa.DIV_MAX_EXCL), ("PG_DIV_MAX_TERMS", "kDivMaxTerms", ref.MAX_TERMS, pa.DIV_MAX_TERMS),
                                       ("PG_DIV_MAX_POSITIONS", "kDivMaxPositions", ref.MAX_POSITIONS, pa.DIV_MAX_POSITIONS),
                                       ("PG_DIV_CHUNK", "kDivChunk", ref.CHUNK, pa.DIV_CHUNK)):
        h = re.search(r"#define\s+%s\s+(\d+)" % macro, hdr)
        k = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % const, hip)
        assert h and k and int(h.group(1)) == int(k.group(1)) == mine == engine, macro
    ops = re.search(r"PG_WHERE_GT = (\d), PG_WHERE_GE = (\d), PG_WHERE_LT = (\d), PG_WHERE_LE = (\d), PG_WHERE_EQ = (\d), PG_WHERE_NE = (\d)", hdr)
    assert [int(x) for x in ops.groups()] == [ref.GT, ref.GE, ref.LT, ref.LE, ref.EQ, ref.NE] == [pa.WHERE_GT, pa.WHERE_GE, pa.WHERE_LT, pa.WHERE_LE,
                                                                                                   pa.WHERE_EQ, pa.WHERE_NE]
    # the structs as the binding lays them out
    assert C.sizeof(_lib.PgDivRule) == 36 and C.sizeof(_lib.PgDivTerm) == 16 and C.sizeof(_lib.PgDivExclusion) == 80
    assert C.sizeof(_lib.PgDivConfig) == 32 + 8 * 36 + 8 * 80 and _lib.PgDivConfig.excl.offset == 320


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------

MIRROR = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [], "SceneConfs": {"home_feed": {"default": {"RecallNames": []}}},
    "SortNames": {"home_feed": ["scatter"]},
    "UserDefineConfs": {"pairec_gpu": {"Device": 0, "Table": {"Rows": 1000, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
                                       "Recalls": [], "Algorithms": [],
                                       "Sorts": [{"Name": "scatter", "SortType": "DiversityRuleSort", "DiversitySize": 50, "ExploreItemSize": 200,
                                                  "ExcludeRecalls": ["hot"],
                                                  "DiversityRules": [{"Dimensions": ["category"], "WindowSize": 10, "FrequencySize": 2, "Weight": 3},
                                                                     {"Dimensions": ["author", "category"], "IntervalSize": 2}],
                                                  "ExclusionRules": [{"Positions": [1, 2, 3],
                                                                      "Conditions": [{"Name": "is_ad", "Type": "int", "Operator": "equal", "Value": 1}]}]}]}},
}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_parse_recconf.restype = C.c_char_p
    L.ph_parse_recconf.argtypes = [C.c_char_p]
    return L


def sorts_of(cfg):
    return cfg["UserDefineConfs"]["pairec_gpu"]["Sorts"]


def test_host_mirror_parses_the_sort(H):
    assert H.ph_parse_recconf(json.dumps(MIRROR).encode()), H.ph_last_error()
    summary = json.loads(H.ph_parse_recconf(json.dumps(MIRROR).encode()))
    assert summary["gpu_sorts"] == 1
    for op in ("equal", "not_equal", "greater", "greaterThan", "less", "lessThan"):
        for typ, value in (("int", 3), ("string", "t1")):
            cfg = copy.deepcopy(MIRROR)
            sorts_of(cfg)[0]["ExclusionRules"][0]["Conditions"][0].update({"Operator": op, "Type": typ, "Value": value})
            served = typ == "int" or op in ("equal", "not_equal")
            assert bool(H.ph_parse_recconf(json.dumps(cfg).encode())) == served, (op, typ, H.ph_last_error())
            if not served:
                assert b"DiversityRuleSort" in H.ph_last_error() and b"integer comparison" in H.ph_last_error()


@pytest.mark.parametrize("edit,word", [
    (lambda s: s.update({"MultiValueDimensionConf": [{"DimensionName": "category", "Delimiter": "/"}]}), b"MultiValueDimensionConf"),
    (lambda s: s["ExclusionRules"][0]["Conditions"][0].update({"Operator": "contains", "Type": "string", "Value": "x"}), b"integer comparison"),
    (lambda s: s["ExclusionRules"][0]["Conditions"][0].update({"Type": "float", "Value": 1.5}), b"integer comparison"),
    (lambda s: s["ExclusionRules"][0]["Conditions"][0].update({"Domain": "user"}), b"integer comparison"),
    (lambda s: s["ExclusionRules"][0].update({"Positions": [0]}), b"position"),
    (lambda s: s["DiversityRules"][0].update({"Dimensions": []}), b"Dimensions"),
    (lambda s: s["DiversityRules"][0].update({"Dimensions": ["a", "b", "c", "d", "e"]}), b"Dimensions"),
    (lambda s: s["DiversityRules"][0].update({"WindowSize": -1}), b"negative"),
    (lambda s: s.update({"DiversityRules": [s["DiversityRules"][0]] * 9}), b"DiversityRules"),
    (lambda s: s.update({"Conditions": [{"Name": "sex", "Domain": "user", "Type": "string", "Operator": "equal", "Value": "f"}]}), b"Conditions"),
])
def test_host_mirror_refuses_by_name(H, edit, word):
    cfg = copy.deepcopy(MIRROR)
    edit(sorts_of(cfg)[0])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    assert b"DiversityRuleSort" in H.ph_last_error() and word in H.ph_last_error(), H.ph_last_error()


def test_host_mirror_keeps_sortconfs_as_they_are(H):
    """SortConfs entries of SortType DiversityRuleSort stay host-side names; only pairec_gpu.Sorts declares the device sort"""
    cfg = copy.deepcopy(MIRROR)
    cfg["SortConfs"] = [{"Name": "host_scatter", "SortType": "DiversityRuleSort", "DiversityRules": [{"Dimensions": ["category"], "IntervalSize": 1}]}]
    assert H.ph_parse_recconf(json.dumps(cfg).encode()), H.ph_last_error()
