"""CPU checks behind ItemStateFilter and BoostScoreSort on the device: tests/cond_ref.py — the specification the
GPU tests compare with — against a literal transcription of the reference's Go code (module/filter_op.go: NewFilterParamWithConfig,
EvaluateByDomain, every operator's Evaluate / DomainEvaluate; sort/boost_score_sort.go:73-104 with its break;
module/item_state_filter_hologres_dao.go's final keep loop) on the reference's own cases (tests/golden/filter_param.json,
tests/golden/boost_score_sort.json) and on random small ones; pg_cond_match_host and pg_boost_scores_host, the host statements of
what the kernels compute, against cond_ref; every refusal; pg_expr_compile_govaluate through the program's host evaluation and
against the feature normalizer's govaluate evaluator."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest

import cond_ref as ref
import pairec_amd as pa
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
MIN_INT32 = -(1 << 31)

with open(os.path.join(ROOT, "tests", "golden", "filter_param.json")) as _f:
    FILTER_CASES = json.load(_f)["cases"]
with open(os.path.join(ROOT, "tests", "golden", "boost_score_sort.json")) as _f:
    BOOST_CASES = json.load(_f)["cases"]


# ---- the reference, literally -------------------------------------------------------------------------------------------------
# Values are what Go would hold: int for int / int32 / int64, float for float64, np.float32 for float32, str, list for []any.

def ToInt(v, default):                                      # utils/type.go:11-42
    if isinstance(v, bool):
        return default
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, np.float32):
        return default                                      # no float32 case
    if isinstance(v, float):
        return int(v)
    if isinstance(v, str):
        try:
            return int(v) if v.strip() == v and v.lstrip("+-").isdigit() else default
        except ValueError:
            return default
    return default


ToInt64 = ToInt


def ToFloat(v, default):                                    # utils/type.go:43-70
    if isinstance(v, bool):
        return default
    if isinstance(v, (int, float, np.integer, np.floating)):
        return float(v)
    if isinstance(v, str):
        try:
            return float(v)
        except ValueError:
            return default
    return default


def ToString(v, default):
    if isinstance(v, str):
        return v
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return str(int(v))
    if isinstance(v, float):
        return repr(v)
    return default


def ToIntArray(v):                                          # utils/type.go:305-328
    return [ToInt(x, 0) for x in v] if isinstance(v, list) else []


def ToStringArray(v):                                       # utils/type.go:330-…: empty strings are dropped from []any
    return [s for s in (ToString(x, "") for x in v) if s != ""] if isinstance(v, list) else []


class _Op:
    domain_op = True                                        # implements FilterByDomainOp

    def __init__(self, config):
        self.Name, self.Type, self.Value = config.get("Name", ""), config.get("Type", ""), config.get("Value")
        self.Domain = config.get("Domain") or "item"
        self.DomainValue = self.Value if isinstance(self.Value, str) else ""

    def OpDomain(self):
        return self.Domain

    # the shape every two-sided DomainEvaluate shares: `conv` is the type's utils.To*, `miss_user` / `miss_item` what the
    # operator returns when the right-hand property is missing, `cmp` the comparison
    def _right(self, conv, default, userProperties, itemProperties, miss_user, miss_item):
        if self.DomainValue == "":
            return True, conv(self.Value, default)
        if self.DomainValue.startswith("user."):
            val = self.DomainValue[5:]
            if val not in userProperties:
                return False, miss_user
            return True, conv(userProperties[val], default)
        if self.DomainValue.startswith("item."):
            val = self.DomainValue[5:]
            if val not in itemProperties:
                return False, miss_item
            return True, conv(itemProperties[val], default)
        return True, conv(self.Value, default)


class EqualFilterOp(_Op):                                   # filter_op.go:31-174
    def Evaluate(self, properties):
        if self.Name not in properties:
            return False
        left = properties[self.Name]
        if self.Type == "string":
            return ToString(left, "v1") == ToString(self.Value, "v2")
        if self.Type == "int":
            return ToInt(left, -1) == ToInt(self.Value, -2)
        if self.Type == "int64":
            return ToInt64(left, -1) == ToInt64(self.Value, -2)
        return False

    def DomainEvaluate(self, properties, userProperties, itemProperties):
        if self.Name not in properties:
            return False
        left = properties[self.Name]
        for type_, conv, dl, dr in (("string", ToString, "v1", "v2"), ("int", ToInt, -1, -2), ("int64", ToInt64, -1, -2)):
            if self.Type == type_:
                v1 = conv(left, dl)
                ok, right = self._right(conv, dr, userProperties, itemProperties, False, False)
                return v1 == right if ok else right
        return False


class NotEqualFilterOp(_Op):                                # :176-317
    def Evaluate(self, properties):
        if self.Name not in properties:
            return True
        left = properties[self.Name]
        if self.Type == "string":
            return ToString(left, "") != ToString(self.Value, "")
        if self.Type == "int":
            return ToInt(left, 0) != ToInt(self.Value, 0)
        if self.Type == "int64":
            return ToInt64(left, 0) != ToInt64(self.Value, 0)
        return False

    def DomainEvaluate(self, properties, userProperties, itemProperties):
        if self.Name not in properties:
            return True
        left = properties[self.Name]
        for type_, conv, d in (("string", ToString, ""), ("int", ToInt, 0), ("int64", ToInt64, 0)):
            if self.Type == type_:
                v1 = conv(left, d)
                ok, right = self._right(conv, d, userProperties, itemProperties, True, True)
                return v1 != right if ok else right
        return False


class InFilterOp(_Op):                                      # :319-451
    def __init__(self, config):
        super().__init__(config)
        self.value = self.DomainValue
        self.int_values = ToIntArray(self.Value) if self.Type == "int" else []
        self.string_values = ToStringArray(self.Value) if self.Type == "string" else []

    def DomainEvaluate(self, properties, userProperties, itemProperties):
        if self.Name not in properties:
            return False
        left = properties[self.Name]
        for type_, conv, d, arr, consts in (("string", ToString, "", ToStringArray, self.string_values), ("int", ToInt, MIN_INT32, ToIntArray, self.int_values)):
            if self.Type == type_:
                v1 = conv(left, d)
                right = []
                if self.value == "":
                    right = consts
                elif self.value.startswith("user."):
                    if self.value[5:] not in userProperties:
                        return False
                    right = arr(userProperties[self.value[5:]])
                elif self.value.startswith("item."):
                    if self.value[5:] not in itemProperties:
                        return True
                    right = arr(itemProperties[self.value[5:]])
                return any(v1 == val for val in right)
        return False

    def Evaluate(self, properties):
        if self.Name not in properties:
            return False
        left = properties[self.Name]
        if self.Type == "string":
            return ToString(left, "") in self.string_values
        if self.Type == "int":
            return ToInt(left, MIN_INT32) in self.int_values
        return False


class NotInFilterOp(_Op):                                   # :1452-1567
    def __init__(self, config):
        super().__init__(config)
        self.value = self.DomainValue
        self.int_values, self.string_values = [], []
        if not isinstance(self.Value, str):
            if self.Type == "int":
                self.int_values = ToIntArray(self.Value)
            elif self.Type == "string":
                self.string_values = ToStringArray(self.Value)

    def Evaluate(self, properties):
        return False

    def DomainEvaluate(self, properties, userProperties, itemProperties):
        if self.Name not in properties:
            return False
        left1 = properties[self.Name]
        for type_, conv, d, arr, consts in (("string", ToString, "", ToStringArray, self.string_values), ("int", ToInt, MIN_INT32, ToIntArray, self.int_values)):
            if self.Type == type_:
                left = conv(left1, d)
                right = []
                if self.value == "":
                    right = consts
                elif self.value.startswith("user."):
                    if self.value[5:] not in userProperties:
                        return True
                    right = arr(userProperties[self.value[5:]])
                elif self.value.startswith("item."):
                    if self.value[5:] not in itemProperties:
                        return True
                    right = arr(itemProperties[self.value[5:]])
                return not any(left == val for val in right)
        return False


def _ordered(cmp, lines):
    class Op(_Op):
        __doc__ = lines

        def Evaluate(self, properties):
            if self.Name not in properties:
                return False
            left = properties[self.Name]
            if self.Type == "float":
                return cmp(ToFloat(left, 0), ToFloat(self.Value, 0))
            if self.Type == "int":
                return cmp(ToInt(left, 0), ToInt(self.Value, 0))
            if self.Type == "int64":
                return cmp(ToInt64(left, 0), ToInt64(self.Value, 0))
            return False

        def DomainEvaluate(self, properties, userProperties, itemProperties):
            if self.Name not in properties:
                return False
            left = properties[self.Name]
            # (float: a missing item.x answers TRUE; int / int64: false — :618-621 against :643-646, and so in all four operators)
            for type_, conv, miss_item in (("float", ToFloat, True), ("int", ToInt, False), ("int64", ToInt64, False)):
                if self.Type == type_:
                    v1 = conv(left, 0)
                    ok, right = self._right(conv, 0, userProperties, itemProperties, False, miss_item)
                    return cmp(v1, right) if ok else right
            return False                                    # ("time" is outside the served types)
    return Op


GreaterFilterOp = _ordered(lambda a, b: a > b, "filter_op.go:542-715")
GreaterThanFilterOp = _ordered(lambda a, b: a >= b, ":717-889")
LessFilterOp = _ordered(lambda a, b: a < b, ":891-1063")
LessThanFilterOp = _ordered(lambda a, b: a <= b, ":1065-1237")


class IsNullFilterOp(_Op):                                  # :1569-1600 — Evaluate only
    domain_op = False

    def Evaluate(self, properties):
        return self.Name not in properties


class IsNotNullFilterOp(_Op):                               # :1602-1633
    domain_op = False

    def Evaluate(self, properties):
        return self.Name in properties


class BoolFilterOp:                                         # :1635-1760
    domain_op = True

    def __init__(self, config):
        v = ToString(config.get("Type", ""), "")
        self.isOrCondition = v == "" or v.lower() == "or"
        self.filterParam = FilterParam(config.get("Configs") or [])

    def OpDomain(self):
        return "item"

    def DomainEvaluate(self, properties, userProperties, itemProperties):
        for op in self.filterParam.operators:
            if op.domain_op:
                if op.OpDomain() == "item":
                    ret = op.DomainEvaluate(itemProperties, userProperties, itemProperties)
                elif op.OpDomain() == "user":
                    ret = op.DomainEvaluate(userProperties, userProperties, itemProperties)
                else:
                    continue
            else:
                if op.OpDomain() == "item":
                    ret = op.Evaluate(itemProperties)
                elif op.OpDomain() == "user":
                    ret = op.Evaluate(userProperties)
                else:
                    raise ValueError("not support this domain:" + op.OpDomain())
            if self.isOrCondition:
                if ret:
                    return True
            elif not ret:
                return False
        return not self.isOrCondition


_OPS = {"equal": EqualFilterOp, "not_equal": NotEqualFilterOp, "in": InFilterOp, "not_in": NotInFilterOp, "greater": GreaterFilterOp,
        "greaterThan": GreaterThanFilterOp, "less": LessFilterOp, "lessThan": LessThanFilterOp, "is_null": IsNullFilterOp,
        "is_not_null": IsNotNullFilterOp, "bool": BoolFilterOp}


class FilterParam:                                          # :453-540
    def __init__(self, configs):
        self.operators = [_OPS[c["Operator"]](c) for c in configs if c.get("Operator") in _OPS]

    def EvaluateByDomain(self, userProperties, itemProperties):
        for op in self.operators:
            if op.domain_op:
                if op.OpDomain() == "item":
                    if not op.DomainEvaluate(itemProperties, userProperties, itemProperties):
                        return False
                elif op.OpDomain() == "user":
                    if not op.DomainEvaluate(userProperties, userProperties, itemProperties):
                        return False
            else:
                if op.OpDomain() == "item":
                    if not op.Evaluate(itemProperties):
                        return False
                elif op.OpDomain() == "user":
                    if not op.Evaluate(userProperties):
                        return False
                else:
                    raise ValueError("not support this domain:" + op.OpDomain())
        return True


def go_boost_sort(config, items, userProperties):
    """BoostScoreSort.doSort (sort/boost_score_sort.go:73-104); items: [{"Score", "Properties"}], scores rewritten in place.
    The expression is evaluated by cond_ref's govaluate subset over the clone of the properties (numbers as float64, as
    govaluate's parameter sanitiser casts them); a name the clone lacks is govaluate's "No parameter found" error.  That makes
    this leg independent of the specification for the walk — matching, the break, the error rule — and NOT for the arithmetic:
    the arithmetic's independent checks are the three golden scores and the 200 expressions against host/feature.cpp below."""
    conditions = [(FilterParam(c.get("Conditions") or []), ref.expr_parse(c["Expression"])) for c in config["BoostScoreConditions"]]
    filterAll = bool(config.get("BoostScoreConditionsFilterAll"))
    applied = []
    for item in items:
        properties = dict(item["Properties"])               # GetCloneFeatures
        last = 0xFF
        for k, (filterParam, expression) in enumerate(conditions):
            if filterParam.EvaluateByDomain(userProperties, properties):
                properties["score"] = item["Score"]
                try:
                    result = ref.expr_eval(expression, properties)
                except (KeyError, TypeError, ValueError):
                    pass                                    # log.Error
                else:
                    item["Score"] = result
                last = k
                if not filterAll:
                    break
        applied.append(last)
    return applied


def go_item_state_keep(filterParam, items, fieldMap, userProperties):
    """the DAO's final loop (item_state_filter_hologres_dao.go:313-357, empty defaultFieldValues, no item cache): an item absent
    from the state table has no properties beyond its own, which here are none; kept iff the FilterParam passes, order kept"""
    kept = []
    for it in items:
        properties = fieldMap.get(it, {})
        if filterParam.EvaluateByDomain(userProperties, properties):
            kept.append(it)
    return kept


# ---- the reference's own cases ------------------------------------------------------------------------------------------------

def _encode_case(c):
    """a golden case → (id-coded config, cols, item_in, user, declared columns) for cond_ref and the C side; strings share one dictionary"""
    d = {}
    sid = lambda s: d.setdefault(s, len(d))                                              # noqa: E731
    cfgs, cols, user, decl = [], {}, {}, []
    item = c["ItemProperties"]
    for f in c["Config"]:
        g = dict(f)
        t = f["Type"]
        conv = (lambda v: sid(v) if isinstance(v, str) else sid(str(v))) if t == "string" else (lambda v: ToInt(v, 0))
        v = f["Value"]
        if isinstance(v, list):
            g["Value"] = [conv(x) for x in (ToStringArray(v) if t == "string" else v)]
        elif isinstance(v, str) and v.startswith("user."):
            if v[5:] in c["UserProperties"]:
                user[v[5:]] = conv(c["UserProperties"][v[5:]])
        elif isinstance(v, str) and v.startswith("item."):
            cols[v[5:]] = np.array([conv(item[v[5:]]) if v[5:] in item else 0], dtype=np.int64)
            decl.append((v[5:], pa.F_I64))
        else:
            g["Value"] = conv(v)
        cols[f["Name"]] = np.array([conv(item[f["Name"]]) if f["Name"] in item else 0], dtype=np.int64)
        decl.append((f["Name"], pa.F_I64))
        cfgs.append(g)
    item_in = np.array([all(f["Name"] in item for f in c["Config"])])
    return cfgs, cols, item_in, user, list(dict(decl).items())


def test_transcription_and_ref_on_the_reference_filter_cases():
    assert len(FILTER_CASES) == 30 and sum(c["served"] for c in FILTER_CASES) == 21
    for c in FILTER_CASES:
        if c["group"] == "not_in":                           # the reference's test calls the operator itself
            got = NotInFilterOp(c["Config"][0]).DomainEvaluate(c["ItemProperties"], c["UserProperties"], c["ItemProperties"])
        else:
            got = FilterParam(c["Config"]).EvaluateByDomain(c["UserProperties"], c["ItemProperties"])
        assert got == c["Expect"], (c["ref"], c["index"])
        if not c["served"]:
            assert c["why_left_out"]
            continue
        cfgs, cols, item_in, user, decl = _encode_case(c)
        assert ref.match(cfgs, 0, cols, item_in, user) == c["Expect"], (c["ref"], c["index"])
        cond = pa.cond_compile([{"Conditions": cfgs}], decl)
        try:
            assert bool(cond.match_host(cols, item_in, user)[0]) == c["Expect"], (c["ref"], c["index"])
        finally:
            cond.free()


def _boost_case_encoded(c):
    names = sorted({k for it in c["items"] for k in it["Properties"]})
    d = {}
    sid = lambda s: d.setdefault(s, len(d))                                              # noqa: E731
    cols = {n: np.array([sid(it["Properties"][n]) for it in c["items"]], dtype=np.int32) for n in names}
    rules = []
    for bc in c["config"]["BoostScoreConditions"]:
        rules.append({"Conditions": [dict(f, Value=sid(f["Value"])) for f in bc["Conditions"]], "Expression": bc["Expression"]})
    return rules, cols, [(n, pa.F_I32) for n in names], np.array([it["Score"] for it in c["items"]], dtype=np.float64)


def test_transcription_ref_and_host_on_the_reference_boost_cases():
    for c in BOOST_CASES:
        items = [dict(it, Properties=dict(it["Properties"])) for it in c["items"]]
        go_boost_sort(c["config"], items, {})
        for k, want in c["expect"].items():
            assert ref.bits(items[int(k)]["Score"]) == ref.bits(want), (c["name"], k, items[int(k)]["Score"])
        rules, cols, decl, score = _boost_case_encoded(c)
        inside = np.ones(len(score), dtype=bool)
        want_s, want_r = ref.boost(rules, False, score, cols, inside, {})
        assert np.array_equal(want_s.view(np.uint64), np.array([it["Score"] for it in items]).view(np.uint64)), c["name"]
        cond = pa.cond_compile(rules, decl, boost=True)
        try:
            got_s, got_r = cond.boost_host(score, cols)
            assert np.array_equal(got_s.view(np.uint64), want_s.view(np.uint64)) and np.array_equal(got_r, want_r), c["name"]
        finally:
            cond.free()
    assert ref.bits(0.93) == ref.bits(ref.expr_eval(ref.expr_parse("round(score * 3, 2)"), {"score": 0.311}))


# ---- random small cases -------------------------------------------------------------------------------------------------------
KINDS = {"i32": (pa.F_I32, np.int32), "i64": (pa.F_I64, np.int64), "f32": (pa.F_F32, np.float32), "f64": (pa.F_F64, np.float64),
         "str": (pa.F_I32, np.int32)}
USERS = {"ui0": "int", "ui1": "int", "uf0": "float", "us0": "str"}
BIG = (1 << 33) + 5


def _rand_case(rng, boost):
    n_cols, n = rng.randint(1, 6), rng.randint(1, 40)
    kinds = [rng.choice(list(KINDS)) for _ in range(n_cols)]
    if not any(k in ("i32", "i64") for k in kinds):
        kinds[0] = "i64"
    names = ["c%d" % k for k in range(n_cols)]
    cols = {}
    for name, kind in zip(names, kinds):
        if kind in ("f32", "f64"):
            cols[name] = np.array([rng.choice([0.0, 0.5, 1.0, 2.0, 2.5, -1.0, 3.25]) for _ in range(n)], dtype=KINDS[kind][1])
        elif kind == "i64":
            cols[name] = np.array([rng.choice([0, 1, 2, 3, 4, -1, BIG, -BIG]) for _ in range(n)], dtype=np.int64)
        else:
            cols[name] = np.array([rng.randint(0, 4) for _ in range(n)], dtype=np.int32)
    by_kind = lambda ks: [nm for nm, k in zip(names, kinds) if k in ks]                  # noqa: E731
    item_in = np.array([rng.random() > 0.25 for _ in range(n)])
    user = {}
    for u, k in USERS.items():
        if rng.random() < 0.7:
            user[u] = rng.choice([0.0, 1.0, 2.5]) if k == "float" else rng.choice([0, 1, 2, 3, BIG])

    def leaf():
        op = rng.choice(["equal", "not_equal", "greater", "greaterThan", "less", "lessThan", "in", "not_in", "is_null", "is_not_null"])
        dom = "user" if rng.random() < 0.25 else rng.choice(["item", ""])
        if op in ("is_null", "is_not_null"):
            return {"Name": rng.choice(list(USERS)) if dom == "user" else rng.choice(names), "Domain": dom, "Operator": op}
        if op in ("equal", "not_equal"):
            ty = rng.choice(["string", "int", "int64", "float"])
        elif op in ("in", "not_in"):
            ty = rng.choice(["string", "int", "int", "int64", "float"])
        else:
            ty = rng.choice(["float", "int", "int64"])
        unread = (ty == "float" and op in ("equal", "not_equal")) or (ty in ("float", "int64") and op in ("in", "not_in"))
        col_kinds = {"string": ("str",), "int": ("i32", "i64"), "int64": ("i32", "i64"), "float": ("i32", "i64", "f32", "f64")}[ty]
        user_kind = {"string": "str", "int": "int", "int64": "int", "float": "float"}[ty]
        pool_c = names if unread else by_kind(col_kinds)
        pool_u = [u for u, k in USERS.items() if k == user_kind]
        if dom == "user":
            name = rng.choice(pool_u)
        elif pool_c:
            name = rng.choice(pool_c)
        else:
            return leaf()
        f = {"Name": name, "Domain": dom, "Operator": op, "Type": ty}
        const = lambda: rng.choice([0.0, 1.0, 2.0, 2.5]) if ty == "float" else rng.choice([0, 1, 2, 3, BIG])      # noqa: E731
        if op in ("in", "not_in"):
            f["Value"] = [const() if ty != "float" else rng.randint(0, 3) for _ in range(rng.choice([0, 1, 2, 3, 6]))]
            return f
        r = rng.random()
        if r < 0.2:
            f["Value"] = "user." + rng.choice(pool_u)
        elif r < 0.4 and pool_c:
            f["Value"] = "item." + rng.choice(pool_c)
        else:
            f["Value"] = const()
        return f

    def conditions():
        out, left = [], rng.randint(0, 5)
        while left > 0:
            if rng.random() < 0.2 and left >= 1:
                kids = [leaf() for _ in range(rng.randint(0, min(3, left - 1)))]
                out.append({"Operator": "bool", "Type": rng.choice(["", "or", "and", "OR", "And"]), "Configs": kids})
                left -= 1 + len(kids)
            else:
                out.append(leaf())
                left -= 1
        return out

    if not boost:
        rules = [{"Conditions": conditions()}]
    else:
        num = by_kind(("i32", "f32", "f64")) or by_kind(("i64",))
        exprs = ["score * 100", "score * (-10)", "round(score * 3, 2)", "round(score * 3)", "score + [%s]" % num[0], "score / %s - 1" % num[-1],
                 "-score ** 2 % 7", "(score + 1.5) * %s ** 2" % num[0], "score % 3 + 0.25", "2 ** 3 * score"]
        rules = [{"Conditions": conditions(), "Expression": rng.choice(exprs)} for _ in range(rng.randint(1, 4))]
    decl = [(nm, KINDS[k][0]) for nm, k in zip(names, kinds)]
    score = np.array([rng.choice([0.0, 0.311, 1.0, -2.5, 7.0, 1e300, math.inf]) for _ in range(n)], dtype=np.float64)
    if rng.random() < 0.2:
        score.view(np.uint64)[rng.randrange(n)] = 0x7FF8000000000ABC      # a NaN with a payload: kept where no rule rewrites it
    return rules, decl, kinds, cols, item_in, user, score


def _go_form(rules, kinds_of, cols, item_in, user):
    """the id-coded case as Go would hold it: strings "s<id>", typed numbers, one property map per item"""
    s = lambda v: "s%d" % v                                                               # noqa: E731

    def cfg(f):
        g = dict(f)
        if f.get("Operator") == "bool":
            g["Configs"] = [cfg(k) for k in f["Configs"]]
        elif f.get("Type") == "string" and "Value" in f and not isinstance(f["Value"], str):
            g["Value"] = [s(v) for v in f["Value"]] if isinstance(f["Value"], list) else s(f["Value"])
        return g

    go_rules = [dict(r, Conditions=[cfg(f) for f in r["Conditions"]]) for r in rules]
    maps = []
    for i in range(len(item_in)):
        m = {}
        if item_in[i]:
            for name, a in cols.items():
                k = kinds_of[name]
                m[name] = s(int(a[i])) if k == "str" else (int(a[i]) if k in ("i32", "i64") else (np.float32(a[i]) if k == "f32" else float(a[i])))
        maps.append(m)
    go_user = {u: (s(v) if USERS[u] == "str" else v) for u, v in user.items()}
    return go_rules, maps, go_user


def test_random_filter_cases_transcription_ref_and_host_agree():
    rng = random.Random(20261018)
    kept_any = 0
    for case in range(2000):
        rules, decl, kinds, cols, item_in, user, _ = _rand_case(rng, boost=False)
        kinds_of = {nm: k for (nm, _), k in zip(decl, kinds)}
        go_rules, maps, go_user = _go_form(rules, kinds_of, cols, item_in, user)
        fp = FilterParam(go_rules[0]["Conditions"])
        want = np.array([fp.EvaluateByDomain(go_user, m) for m in maps])
        got_ref = np.array([ref.match(rules[0]["Conditions"], i, cols, item_in, user) for i in range(len(item_in))])
        assert np.array_equal(got_ref, want), (case, rules)
        # the DAO's keep loop = the order-preserving keep of the matches
        ids = list(range(len(item_in)))
        assert go_item_state_keep(fp, ids, {i: m for i, m in enumerate(maps) if item_in[i]}, go_user) == [i for i in ids if want[i]]
        cond = pa.cond_compile(rules, decl)
        try:
            assert np.array_equal(cond.match_host(cols, item_in, user, n=len(item_in)), want), (case, rules)
        finally:
            cond.free()
        kept_any += int(want.any())
    assert kept_any > 300


def test_random_boost_cases_transcription_ref_and_host_agree():
    rng = random.Random(7)
    rewritten = 0
    for case in range(1200):
        rules, decl, kinds, cols, item_in, user, score = _rand_case(rng, boost=True)
        filter_all = case % 2 == 1
        kinds_of = {nm: k for (nm, _), k in zip(decl, kinds)}
        go_rules, maps, go_user = _go_form(rules, kinds_of, cols, item_in, user)
        items = [{"Score": float(sc), "Properties": m} for sc, m in zip(score, maps)]
        applied = go_boost_sort({"BoostScoreConditions": go_rules, "BoostScoreConditionsFilterAll": filter_all}, items, go_user)
        want_s = ref.score_bits(np.array([it["Score"] for it in items], dtype=np.float64))
        ref_s, ref_r = ref.boost(rules, filter_all, score, cols, item_in, user)
        assert np.array_equal(ref.score_bits(ref_s), want_s) and list(ref_r) == applied, (case, rules)
        cond = pa.cond_compile(rules, decl, boost=True)
        try:
            got_s, got_r = cond.boost_host(score, cols, item_in, user, filter_all)
            assert np.array_equal(ref.score_bits(got_s), want_s) and np.array_equal(got_r, ref_r), (case, rules)
            untouched = got_r == 0xFF                            # no rule matched: the very bits
            assert np.array_equal(got_s.view(np.uint64)[untouched], score.view(np.uint64)[untouched])
        finally:
            cond.free()
        rewritten += int((ref_r != 0xFF).any())
    assert rewritten > 300


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def _refused(code, word, rules, cols=(("a", pa.F_I32), ("f", pa.F_F32), ("s", pa.F_I32)), boost=False):
    with pytest.raises(PgError) as ei:
        pa.cond_compile(rules, list(cols), boost=boost)
    assert ei.value.code == code and word in str(ei.value), (rules, str(ei.value))


def test_every_refusal_returns_its_code_and_names_the_offender():
    t = lambda **kw: {"Conditions": [dict({"Name": "a", "Operator": "equal", "Type": "int", "Value": 1}, **kw)]}      # noqa: E731
    _refused(UNSUPPORTED, '"contains"', [t(Operator="contains", Value="user.x")])
    _refused(UNSUPPORTED, '"not_contains"', [t(Operator="not_contains", Value="user.x")])
    _refused(UNSUPPORTED, '"expression"', [t(Operator="expression", Value="a > 1")])
    _refused(UNSUPPORTED, '"s"', [t(Name="s", Operator="greater", Type="string", Value=3)])
    _refused(UNSUPPORTED, '"f"', [t(Name="f", Operator="equal", Type="int")])
    _refused(UNSUPPORTED, '"f"', [t(Name="f", Operator="less", Type="int64")])
    _refused(UNSUPPORTED, '"f"', [t(Operator="greater", Type="int", Value="item.f")])
    _refused(UNSUPPORTED, "user.tags", [t(Operator="in", Value="user.tags")])
    _refused(UNSUPPORTED, "user.tags", [t(Operator="not_in", Type="string", Name="s", Value="user.tags")])
    _refused(UNSUPPORTED, "deeper than one bool", [{"Conditions": [{"Operator": "bool", "Configs": [{"Operator": "bool", "Configs": []}]}]}])
    _refused(UNSUPPORTED, "deeper than one bool", [{"Conditions": [{"Operator": "bool", "Configs": [{"Operator": "bool", "Configs": [
        {"Name": "a", "Operator": "is_null"}]}]}]}])
    _refused(UNSUPPORTED, '"context"', [t(Domain="context")])
    _refused(UNSUPPORTED, '"context"', [t(Domain="context", Operator="is_null")])
    _refused(UNSUPPORTED, "9 rules", [t()] * 9)
    _refused(UNSUPPORTED, "9 operators", [{"Conditions": [t()["Conditions"][0]] * 9}])
    _refused(UNSUPPORTED, "9 operators", [{"Conditions": [{"Operator": "bool", "Configs": [t()["Conditions"][0]] * 8}]}])
    _refused(UNSUPPORTED, "65 values", [t(Operator="in", Value=list(range(65)))])
    _refused(UNSUPPORTED, "user slots", [{"Conditions": [dict(t()["Conditions"][0], Domain="user", Name="u%d" % k) for k in range(5)]},
                                         {"Conditions": [dict(t()["Conditions"][0], Domain="user", Name="v%d" % k) for k in range(4)]}])
    many = [("c%d" % k, pa.F_I32) for k in range(17)]
    _refused(UNSUPPORTED, "referenced columns", [{"Conditions": [dict(t()["Conditions"][0], Name="c%d" % (8 * r + k)) for k in range(8)]}
                                                 for r in range(3)], cols=many)
    _refused(UNSUPPORTED, '"score"', [dict(t(Name="score"), Expression="score * 2")], cols=(("score", pa.F_F64),), boost=True)
    _refused(UNSUPPORTED, "item.score", [dict(t(Operator="greater", Type="float", Value="item.score"), Expression="score * 2")],
             cols=(("a", pa.F_I32), ("score", pa.F_F64)), boost=True)
    _refused(INVALID, "without an expression", [t()], boost=True)
    _refused(INVALID, "without an expression", [dict(t(), Expression="")], boost=True)
    _refused(INVALID, "not a boost rule set", [dict(t(), Expression="score")])
    _refused(INVALID, '"nobody"', [t(Name="nobody")])
    _refused(INVALID, '"nobody"', [dict(t(), Expression="score * nobody")], boost=True)
    _refused(INVALID, '"u"', [{"Conditions": [dict(t()["Conditions"][0], Domain="user", Name="u"),
                                              dict(t()["Conditions"][0], Domain="user", Name="u", Operator="less", Type="float", Value=1.5)]}])
    _refused(UNSUPPORTED, "'>'", [dict(t(), Expression="score > 1")], boost=True)
    _refused(UNSUPPORTED, "depth", [dict(t(), Expression="1+(2+(3+(4+(5+(6+(7+(8+(9+score))))))))")], boost=True)
    with pytest.raises(ValueError):
        pa.cond_compile([t(Type="time", Operator="greater")], [("a", pa.F_I32)])
    # served on the edge of the limits: 8 rules of 8 operators, 64 values, an empty FilterParam, score as a user property
    c = pa.cond_compile([{"Conditions": [{"Operator": "bool", "Type": "and", "Configs": [t(Operator="in", Value=list(range(64)))["Conditions"][0]] * 7}]}] * 8,
                        [("a", pa.F_I32)])
    assert c.n_rules == 8
    c.free()
    c = pa.cond_compile([{"Conditions": []}], [])
    assert c.match_host(n=3).all()
    c.free()
    c = pa.cond_compile([{"Conditions": [{"Name": "score", "Domain": "user", "Operator": "greater", "Type": "float", "Value": 0.5}],
                          "Expression": "score"}], [], boost=True)
    assert c.user_slots == [("score", True)]
    c.free()


def test_header_limits_match_the_build():
    src = open(os.path.join(ROOT, "include", "pairec_gpu.h")).read()
    for name, val in (("RULES", pa.COND_MAX_RULES), ("TERMS", pa.COND_MAX_TERMS), ("COLS", pa.COND_MAX_COLS), ("SLOTS", pa.COND_MAX_SLOTS),
                      ("LIST", pa.COND_MAX_LIST)):
        assert "#define PG_COND_MAX_%s %d\n" % (name, val) in src


# ---- pg_expr_compile_govaluate ------------------------------------------------------------------------------------------------

def _gv(source, **env):
    e = pa.expr_compile_govaluate(source)
    try:
        v = np.array([[float(env[n])] for n in e.var_names], dtype=np.float64).reshape(len(e.var_names), 1)
        return float(e.eval_host(v)[0])
    finally:
        e.free()


def test_govaluate_parse_precedence_and_round():
    assert _gv("2 ** 3 * 2") == 16.0
    assert _gv("-score ** 2", score=3.0) == 9.0                 # the prefix binds tighter than **
    assert _gv("-(score ** 2)", score=3.0) == -9.0
    assert _gv("7 % 3") == 1.0 and _gv("7.5 % 2") == 1.5 and _gv("-7 % 3") == -1.0 and math.isnan(_gv("7 % 0"))
    assert _gv("1 / 0") == math.inf and _gv("-1 / 0") == -math.inf and math.isnan(_gv("0 / 0"))
    assert _gv("1 + 2 * 3 - 4 / 8") == 6.5 and _gv("(1 + 2) * 3") == 9.0 and _gv("2 * -3") == -6.0 and _gv("10 - 2 - 3") == 5.0
    assert _gv("score * (-10)", score=10.0) == -100.0 and _gv("[my score] + 1", **{"my score": 2.0}) == 3.0
    assert ref.bits(_gv("round(score * 3, 2)", score=0.311)) == ref.bits(0.93)
    assert _gv("round(score * 3)", score=0.311) == 1.0
    assert _gv("round(2.5)") == 3.0 and _gv("round(-2.5)") == -3.0 and _gv("round(-0.4)") == 0.0
    assert _gv("round(1234.5678, -2)") == 1200.0 and _gv("round(-1.239, 2)") == -1.23
    e = pa.expr_compile_govaluate("a + [b c] * a + score")
    assert e.var_names == ["a", "b c", "score"]
    e.free()
    pa.expr_compile_govaluate("").free()
    for bad, word in (("score > 1", "'>'"), ("a == b", "'=='"), ("a ? 1 : 2", "'?'"), ("a && b", "'&&'"), ("a || b", "'||'"), ("'x'", "string"),
                      ("log(a)", '"log"'), ("max(a, b)", '"max"'), ("2 ** 3 ** 2", "chained"), ("1e5", "malformed number"), ("a.b", '"a.b"'),
                      ("true", '"true"'), ("!a", "'!'"), ("(1, 2)", "array"), ("a in (1, 2)", '"in"'), ("round(1, 2, 3)", "wrong number"),
                      ("(a", "')'"), ("a +", "end of the expression"), ("0x10", "hexadecimal"), ("a & b", "'&'"), ("~a", "'~'")):
        with pytest.raises(PgError) as ei:
            pa.expr_compile_govaluate(bad)
        assert ei.value.code == UNSUPPORTED and word in str(ei.value) and "subset" in str(ei.value), (bad, str(ei.value))
    # the other two front ends keep their grammars
    e = pa.Expr("${a} # ${b} % 3", "default")
    assert e.var_names == ["a", "b"] and e.eval_host(np.array([[0.0], [7.0]]))[0] == 1.0
    e.free()
    e = pa.Expr("-(${a}^2)", "antlr")
    assert e.eval_host(np.array([[3.0]]))[0] == -9.0
    e.free()


@pytest.fixture(scope="module")
def HOST():
    L = C.CDLL(os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_normalizer_apply.restype = C.c_char_p
    L.ph_normalizer_apply.argtypes = [C.c_char_p]
    return L


def _rand_expr(rng, depth=0):
    r = rng.random()
    if depth >= 3 or r < 0.3:
        return rng.choice(["score", "a", "[b b]", "2", "0.5", "3.25", "10", "7", "0"])
    if r < 0.4:
        return "-" + _rand_expr(rng, depth + 1) if rng.random() < 0.5 else "(" + _rand_expr(rng, depth + 1) + ")"
    if r < 0.5:
        return "round(%s)" % _rand_expr(rng, depth + 1) if rng.random() < 0.5 else "round(%s, %d)" % (_rand_expr(rng, depth + 1), rng.randint(0, 3))
    if r < 0.58:
        # ** where both evaluators restate Go's Pow: a small integer exponent of an exactly representable base (the products are exact)
        return "(%s ** %d)" % (rng.choice(["2", "0.5", "3", "a", "10"]), rng.randint(0, 4))
    return "(%s %s %s)" % (_rand_expr(rng, depth + 1), rng.choice(["+", "-", "*", "/", "%"]), _rand_expr(rng, depth + 1))


def test_govaluate_agrees_with_the_feature_normalizer_evaluator(HOST):
    rng = random.Random(99)
    done = 0
    while done < 200:
        src = _rand_expr(rng)
        env = {"score": rng.choice([0.311, 2.0, -1.5, 100.0]), "a": rng.choice([3.0, 0.0, -2.0, 4.0]), "b b": rng.choice([0.25, 7.0, 1e6])}
        r = HOST.ph_normalizer_apply(json.dumps(dict(name="expression", expression=src, value=env)).encode())
        assert r is not None, (src, HOST.ph_last_error())
        want = json.loads(r)["result"]
        e = pa.expr_compile_govaluate(src)
        try:
            got = float(e.eval_host(np.array([[env[n]] for n in e.var_names], dtype=np.float64).reshape(len(e.var_names), 1))[0])
        finally:
            e.free()
        mine = ref.expr_eval(ref.expr_parse(src), env)
        assert ref.bits(got) == ref.bits(mine) or (math.isnan(got) and math.isnan(mine)), (src, env, got, mine)
        if want is None or isinstance(want, str):               # JSON has no NaN / Inf: the mirror prints those as null or text
            assert not math.isfinite(got), (src, env, got, want)
        else:
            assert ref.bits(float(want)) == ref.bits(got) or (want == 0 and got == 0), (src, env, got, want)
        done += 1
