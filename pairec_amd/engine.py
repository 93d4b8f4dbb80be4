"""Thin object layer over the C ABI (include/pairec_gpu.h): Context, Table, RankModel, Expr.

Host arrays are numpy; "dev" methods take raw device addresses (ints), e.g. torch tensors'
`.data_ptr()` — torch is used by callers only as plumbing for device memory and RCCL.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib

PREC_F32, PREC_BF16, PREC_BF16X3, PREC_F16X2, PREC_F16 = 0, 1, 2, 3, 4
MODEL_DNN3, MODEL_FM_TWOTOWER, MODEL_DNN3_MULTI = 1, 2, 3
MAX_QUERIES = 256         # per table pass (32 when dim > 128)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _pack_lists(lists, nq: int):
    """one exclusion list per request → (ids uint64 [total], offsets uint32 [nq + 1]); None = every list empty"""
    if lists is None:
        lists = [()] * nq
    if len(lists) != nq:
        raise ValueError("%d exclusion lists for %d requests" % (len(lists), nq))
    arrs = [np.asarray(l, dtype=np.uint64).reshape(-1) for l in lists]
    off = np.zeros(nq + 1, dtype=np.uint32)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    ids = np.ascontiguousarray(np.concatenate(arrs)) if nq else np.zeros(0, dtype=np.uint64)
    return ids, off


TRIM_FIX, TRIM_ACCUMULATE, TRIM_ANY = 0, 1, 0xFF


def _trim_rules(rules):
    arr = (_lib.PgTrimRule * max(len(rules), 1))()
    for i, (source, type_, count) in enumerate(rules):
        arr[i] = _lib.PgTrimRule(int(source), int(type_), int(count))
    return arr


def trim_out_cap(rules, cap: int) -> int:
    """pg_trim_out_cap: rules = [(source, TRIM_FIX | TRIM_ACCUMULATE, count)] → min(cap, the FIX counts + the largest ACCUMULATE
    count); raises PgError for a rule set the trim refuses.  A host function: no context, no device."""
    out = C.c_uint32()
    _lib.check(_lib.load().pg_trim_out_cap(_trim_rules(rules), len(rules), int(cap), C.byref(out)))
    return out.value


def trim2_out_cap(rules, cap: int) -> int:
    """pg_trim2_out_cap: rules = [(source, TRIM_FIX | TRIM_ACCUMULATE, count)] for PriorityAdjustCountFilterV2 → min(cap, the FIX
    counts + the largest ACCUMULATE count); raises PgError for a rule set the call refuses.  A host function: no context, no
    device."""
    out = C.c_uint32()
    _lib.check(_lib.load().pg_trim2_out_cap(_trim_rules(rules), len(rules), int(cap), C.byref(out)))
    return out.value


BLEND_SNAKE_REFILL, BLEND_SNAKE_SKIP, BLEND_FAIR = 0, 1, 2


def _blend_conf(conf):
    """conf = (mode, retain_num, [(source, weight)]) → pg_blend_conf (entries the struct cannot hold are left to the library's
    n_entries check)"""
    mode, retain_num, entries = conf
    entries = list(entries or ())
    c = _lib.PgBlendConf(int(mode), int(retain_num), len(entries))
    for i, (source, weight) in enumerate(entries[:8]):
        c.source[i] = int(source)
        c.weight[i] = int(weight)
    return c


def blend_out_cap(conf, cap: int) -> int:
    """pg_blend_out_cap: conf = (BLEND_SNAKE_REFILL | BLEND_SNAKE_SKIP | BLEND_FAIR, retain_num, [(source, weight)]) →
    min(cap, retain_num); raises PgError for a conf the blend refuses.  A host function: no context, no device."""
    out = C.c_uint32()
    _lib.check(_lib.load().pg_blend_out_cap(C.byref(_blend_conf(conf)), int(cap), C.byref(out)))
    return out.value


def _cand_arrays(who, out_cap_of, rows, score, source, count, planes_f64, source_mask, planes_f32):
    """a request batch's candidate lists on host arrays, checked and made contiguous; out_cap_of: cap → the outputs' width →
    (nq, cap, [rows, score, source, count, planes_f64, source_mask, planes_f32], outs, n64, n32)"""
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    sc = np.ascontiguousarray(score, dtype=np.float64)
    if r.ndim != 2 or sc.shape != r.shape:
        raise ValueError("%s: rows and score are [nq][cap]" % who)
    nq, cap = r.shape
    out_cap = out_cap_of(cap)
    opt = [None if source is None else np.ascontiguousarray(source, dtype=np.uint8),
           None if count is None else np.ascontiguousarray(count, dtype=np.uint32),
           None if planes_f64 is None else np.ascontiguousarray(planes_f64, dtype=np.float64),
           None if source_mask is None else np.ascontiguousarray(source_mask, dtype=np.uint32),
           None if planes_f32 is None else np.ascontiguousarray(planes_f32, dtype=np.float32)]
    for a, shape in ((opt[0], (nq, cap)), (opt[1], (nq,)), (opt[3], (nq, cap))):
        if a is not None and a.shape != shape:
            raise ValueError("%s: source and source_mask are [nq][cap], count [nq]" % who)
    for a in (opt[2], opt[4]):
        if a is not None and (a.ndim != 3 or a.shape[1:] != (nq, cap)):
            raise ValueError("%s: planes are [n][nq][cap]" % who)
    n64 = opt[2].shape[0] if opt[2] is not None else 0
    n32 = opt[4].shape[0] if opt[4] is not None else 0
    outs = [np.empty((nq, out_cap), np.uint64), np.empty((nq, out_cap), np.float64),
            None if opt[0] is None else np.empty((nq, out_cap), np.uint8),
            None if opt[2] is None else np.empty((n64, nq, out_cap), np.float64),
            None if opt[3] is None else np.empty((nq, out_cap), np.uint32),
            None if opt[4] is None else np.empty((n32, nq, out_cap), np.float32), np.empty(nq, np.uint32)]
    return nq, cap, [r, sc] + opt, outs, n64, n32


def candidates_blend_host(conf, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """pg_candidates_blend_host: SnakeFilter / CompletelyFairCountFilter on host arrays by the library's host statement (no
    context, no device); arguments and result as Context.candidates_blend."""
    nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_blend_host", lambda cap: blend_out_cap(conf, cap), rows, score, source, count,
                                                planes_f64, source_mask, planes_f32)
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_candidates_blend_host(C.byref(_blend_conf(conf)), nq, cap, v(ins[0]), v(ins[1]), v(ins[2]), v(ins[3]),
                                                    v(ins[4]), n64, v(ins[5]), v(ins[6]), n32, *[v(a) for a in outs]))
    return tuple(outs)


def candidates_trim2_host(rules, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """pg_candidates_trim2_host: PriorityAdjustCountFilterV2 on host arrays by the library's host statement (no context, no
    device); arguments and result as Context.candidates_trim2."""
    nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_trim2_host", lambda cap: trim2_out_cap(rules, cap), rows, score, source, count,
                                                planes_f64, source_mask, planes_f32)
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_candidates_trim2_host(_trim_rules(rules), len(rules), nq, cap, v(ins[0]), v(ins[1]), v(ins[2]), v(ins[3]),
                                                    v(ins[4]), n64, v(ins[5]), v(ins[6]), n32, *[v(a) for a in outs]))
    return tuple(outs)


DIV_MAX_N, DIV_MAX_RULES, DIV_MAX_DIMS, DIV_MAX_COLS, DIV_MAX_EXCL, DIV_MAX_TERMS, DIV_MAX_POSITIONS, DIV_CHUNK = 8192, 8, 4, 16, 8, 4, 64, 1024
WHERE_GT, WHERE_GE, WHERE_LT, WHERE_LE, WHERE_EQ, WHERE_NE = range(6)


def _div_config(cfg, n_cols: int):
    """a DiversityRuleSort config → (pg_div_config, the arrays it points to).  cfg: {"size", "diversity_size", "explore_item_size",
    "exclude_source_mask", "rules": [{"dims": [column indices], "interval", "window", "frequency", "weight"}], "exclusions":
    [{"positions": [1-based], "terms": [(column, WHERE_*, value)]}], "multi_value": MultiValueDimensionConf entries}; absent keys
    are 0 / empty.  More entries than the C arrays hold are cut here and still counted, so the C side refuses them."""
    c = _lib.PgDivConfig()
    c.size, c.diversity_size = int(cfg.get("size", 0)), int(cfg.get("diversity_size", 0))
    c.explore_item_size, c.exclude_source_mask = int(cfg.get("explore_item_size", 0)), int(cfg.get("exclude_source_mask", 0))
    c.n_cols, c.n_multi_value = int(cfg.get("n_cols", n_cols)), int(cfg.get("multi_value", 0))
    rules, excl, keep = list(cfg.get("rules", ())), list(cfg.get("exclusions", ())), []
    c.n_rules, c.n_excl = len(rules), len(excl)
    for i, r in enumerate(rules[:DIV_MAX_RULES]):
        dims = list(r.get("dims", ()))
        c.rules[i].n_dims = len(dims)
        for k, d in enumerate(dims[:DIV_MAX_DIMS]):
            c.rules[i].dims[k] = int(d)
        c.rules[i].interval, c.rules[i].window = int(r.get("interval", 0)), int(r.get("window", 0))
        c.rules[i].frequency, c.rules[i].weight = int(r.get("frequency", 0)), int(r.get("weight", 0))
    for i, e in enumerate(excl[:DIV_MAX_EXCL]):
        pos = np.ascontiguousarray(list(e.get("positions", ())), dtype=np.uint32)
        keep.append(pos)
        c.excl[i].positions = pos.ctypes.data_as(C.POINTER(C.c_uint32)) if pos.size else None
        c.excl[i].n_positions = pos.size
        terms = list(e.get("terms", ()))
        c.excl[i].n_terms = len(terms)
        for k, (col, op, value) in enumerate(terms[:DIV_MAX_TERMS]):
            c.excl[i].terms[k] = _lib.PgDivTerm(int(col), int(op), int(value))
    return c, keep


def _div_planes(dims, count, source, enable):
    d = np.ascontiguousarray(dims, dtype=np.int64)
    if d.ndim != 3:
        raise ValueError("diversity_rules: dims is [n_cols][nq][cap]")
    n_cols, nq, cap = d.shape
    cnt = None if count is None else np.ascontiguousarray(count, dtype=np.uint32)
    src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8)
    en = None if enable is None else np.ascontiguousarray(enable, dtype=np.uint8)
    if (cnt is not None and cnt.shape != (nq,)) or (en is not None and en.shape != (nq,)) or (src is not None and src.shape != (nq, cap)):
        raise ValueError("diversity_rules: count and enable are [nq], source [nq][cap]")
    return d, n_cols, nq, cap, cnt, src, en


def diversity_rules_host(cfg, dims, count=None, source=None, enable=None) -> np.ndarray:
    """pg_diversity_rules_host: DiversityRuleSort of nq requests on the host — the statement the kernel reproduces (no context, no
    device).  dims [n_cols][nq][cap] int64 → order [nq][cap] uint32 (UINT32_MAX behind count)."""
    d, n_cols, nq, cap, cnt, src, en = _div_planes(dims, count, source, enable)
    c, keep = _div_config(cfg, n_cols)
    out = np.empty((nq, cap), dtype=np.uint32)
    o = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_diversity_rules_host(C.byref(c), nq, cap, o(cnt), _ptr(d), o(src), o(en), _ptr(out)))
    del keep
    return out


COND_MAX_RULES, COND_MAX_TERMS, COND_MAX_COLS, COND_MAX_SLOTS, COND_MAX_LIST = 8, 8, 16, 8, 64
_COND_OPS = {"equal": 0, "not_equal": 1, "greater": 2, "greaterThan": 3, "less": 4, "lessThan": 5, "in": 6, "not_in": 7,
             "is_null": 8, "is_not_null": 9, "bool": 10, "contains": 11, "not_contains": 12, "expression": 13}
_COND_TYPES = {"int": 0, "int64": 1, "float": 2, "string": 3}
_F_NP = {1: np.int32, 2: np.int64, 3: np.float32, 4: np.float64}


def _cond_const(value, type_, strings):
    """a FilterParamConfig.Value as the term's constant: utils.ToInt / ToInt64 / ToFloat of a JSON value (numbers, numeric strings),
    the dictionary id of a string"""
    if type_ == "string":
        if isinstance(value, str):
            if value not in strings:
                strings[value] = -2 - len(strings)          # a value no item carries: an id no dictionary hands out
            return int(strings[value]), 0.0
        return int(value), 0.0                              # already a dictionary id
    if type_ == "float":
        return 0, float(value)
    return int(float(value)) if isinstance(value, (float, str)) else int(value), 0.0


def _cond_terms(configs, strings, keep, depth=0):
    """[FilterParamConfig] (the reference's JSON keys: Name, Domain, Operator, Type, Value, Configs) → [PgCondTerm], a bool
    followed by its children.  As NewFilterParamWithConfig (filter_op.go:457-495) an unknown Operator adds nothing."""
    out = []
    for cfg in configs:
        op = cfg.get("Operator", "")
        if op not in _COND_OPS:
            continue
        t = _lib.PgCondTerm()
        t.op, t.depth = _COND_OPS[op], depth
        keep.append((cfg.get("Name", "") or "").encode("utf-8"))
        t.name = keep[-1]
        keep.append((cfg.get("Domain", "") or "").encode("utf-8"))
        t.domain = keep[-1]
        if op == "bool":
            ty = str(cfg.get("Type", "") or "")
            t.bool_and = 0 if ty == "" or ty.lower() == "or" else 1           # NewBoolFilterOp, :1640-1651
            out.append(t)
            out.extend(_cond_terms(cfg.get("Configs", ()) or (), strings, keep, depth + 1))
            continue
        ty = cfg.get("Type", "")
        if op in ("is_null", "is_not_null"):
            out.append(t)
            continue
        if ty not in _COND_TYPES:
            raise ValueError("FilterParam: Type %r of %r is not served (int, int64, float, string)" % (ty, cfg.get("Name")))
        t.type = _COND_TYPES[ty]
        v = cfg.get("Value")
        if isinstance(v, str) and (v.startswith("user.") or v.startswith("item.")):
            t.rhs = 1 if v.startswith("user.") else 2
            keep.append(v[5:].encode("utf-8"))
            t.rhs_name = keep[-1]
        elif op in ("in", "not_in"):
            vals = [] if v is None or isinstance(v, str) else [_cond_const(x, "int" if ty != "string" else ty, strings)[0] for x in v]
            arr = (C.c_longlong * max(len(vals), 1))(*vals)
            keep.append(arr)
            t.list, t.n_list = arr, len(vals)
        elif op not in ("contains", "not_contains", "expression"):
            t.i, t.f = _cond_const(v, ty, strings)
        out.append(t)
    return out


class Cond:
    """A compiled condition set (pg_cond_compile): 1..8 FilterParams over declared columns, optionally each with a govaluate
    expression (a BoostScoreSort rule set).  rules: [{"Conditions": [FilterParamConfig], "Expression": str}] with the
    reference's JSON keys; cols: [(name, F_I32 | F_I64 | F_F32 | F_F64)]; strings: {value: dictionary id} for string terms
    (a value it lacks gets an id no item carries).  A host object until a device entry first uses it."""

    def __init__(self, rules, cols, boost: bool = False, strings: Optional[dict] = None):
        self.L = _lib.load()
        self.cols = [(str(n), int(d)) for n, d in cols]
        self.boost = bool(boost)
        self.strings = dict(strings or {})
        keep = []
        arr = (_lib.PgCondRule * max(len(rules), 1))()
        for i, r in enumerate(rules):
            terms = _cond_terms(r.get("Conditions", ()) or (), self.strings, keep)
            ta = (_lib.PgCondTerm * max(len(terms), 1))(*terms)
            keep.append(ta)
            arr[i].terms, arr[i].n_terms = ta, len(terms)
            if r.get("Expression") is not None:
                keep.append(str(r["Expression"]).encode("utf-8"))
                arr[i].expression = keep[-1]
        ca = (_lib.PgCondCol * max(len(self.cols), 1))()
        for i, (n, d) in enumerate(self.cols):
            keep.append(n.encode("utf-8"))
            ca[i].name, ca[i].dtype = keep[-1], d
        h = C.c_void_p()
        _lib.check(self.L.pg_cond_compile(arr, len(rules), ca, len(self.cols), 1 if boost else 0, C.byref(h)))
        del keep
        self.h = h
        self.n_rules = self.L.pg_cond_num_rules(h)
        self.user_slots = [(self.L.pg_cond_user_slot_name(h, i).decode("utf-8"), bool(self.L.pg_cond_user_slot_is_float(h, i)))
                           for i in range(self.L.pg_cond_num_user_slots(h))]

    def free(self):
        if self.h:
            self.L.pg_cond_free(self.h)
            self.h = None

    def pack_user(self, users):
        """one {name: value} per request (a name it lacks: the slot is absent) → (vals [nq][8] uint64 bits, present [nq] uint32)"""
        vals = np.zeros((len(users), COND_MAX_SLOTS), dtype=np.uint64)
        present = np.zeros(len(users), dtype=np.uint32)
        for q, u in enumerate(users):
            for s, (name, is_float) in enumerate(self.user_slots):
                if u is not None and name in u:
                    present[q] |= np.uint32(1 << s)
                    vals[q, s] = np.array([u[name]], dtype=np.float64 if is_float else np.int64).view(np.uint64)[0]
        return vals, present

    def _host_args(self, cols, item_in, user):
        n, arrs = None, []
        ptrs = (C.c_void_p * max(len(self.cols), 1))()
        for i, (name, dt) in enumerate(self.cols):
            if cols is not None and name in cols:
                a = np.ascontiguousarray(cols[name], dtype=_F_NP[dt]).reshape(-1)
                arrs.append(a)
                ptrs[i] = a.ctypes.data
                n = a.shape[0] if n is None else n
                if a.shape[0] != n:
                    raise ValueError("Cond: the columns' arrays differ in length")
        inn = None if item_in is None else np.ascontiguousarray(item_in, dtype=np.uint8).reshape(-1)
        if inn is not None:
            n = inn.shape[0] if n is None else n
        vals, present = self.pack_user([user])
        return n, arrs, ptrs, inn, vals, int(present[0])

    def match_host(self, cols=None, item_in=None, user=None, rule: int = 0, n: Optional[int] = None) -> np.ndarray:
        """pg_cond_match_host: rule `rule` on n candidates given as candidate-aligned arrays {column name: [n]}; item_in [n]:
        0 = the candidate's row is outside the store; user {name: value} of the one request → [n] bool."""
        m, arrs, ptrs, inn, vals, present = self._host_args(cols, item_in, user)
        n = m if n is None else n
        out = np.zeros(n or 0, dtype=np.uint8)
        _lib.check(self.L.pg_cond_match_host(self.h, rule, n or 0, None if inn is None else _ptr(inn), ptrs, _ptr(vals), present, _ptr(out)))
        del arrs
        return out.astype(bool)

    def boost_host(self, score, cols=None, item_in=None, user=None, filter_all: bool = False):
        """pg_boost_scores_host: BoostScoreSort's walk on n candidates → (scores [n] fp64, last matching rule [n] uint8, 0xFF none)"""
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        m, arrs, ptrs, inn, vals, present = self._host_args(cols, item_in, user)
        if m is not None and m != sc.shape[0]:
            raise ValueError("Cond.boost_host: score and the columns differ in length")
        out, rule = np.empty_like(sc), np.empty(sc.shape[0], dtype=np.uint8)
        _lib.check(self.L.pg_boost_scores_host(self.h, 1 if filter_all else 0, sc.shape[0], None if inn is None else _ptr(inn), ptrs, _ptr(vals),
                                               present, _ptr(sc), _ptr(out), _ptr(rule)))
        del arrs
        return out, rule


def cond_compile(rules, cols, boost: bool = False, strings: Optional[dict] = None) -> Cond:
    """pg_cond_compile (see Cond)."""
    return Cond(rules, cols, boost, strings)


def cond_match_host(cond: Cond, cols=None, item_in=None, user=None, rule: int = 0, n: Optional[int] = None) -> np.ndarray:
    """pg_cond_match_host (see Cond.match_host): a host function, no context, no device."""
    return cond.match_host(cols, item_in, user, rule, n)


def distinct_ids_host(cond: Cond, ids, cols=None, item_in=None, user=None, n: Optional[int] = None) -> np.ndarray:
    """pg_distinct_ids_host: DistinctIdSort's ids of the n candidates of one request, given as Cond.match_host's arguments; ids: one
    int64 per rule of the set → [n] int64 (the first matching rule's id, else position + 1).  A host function, no device."""
    di = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    if di.shape[0] != cond.n_rules:
        raise ValueError("distinct_ids_host: %d ids for %d rules" % (di.shape[0], cond.n_rules))
    m, arrs, ptrs, inn, vals, present = cond._host_args(cols, item_in, user)
    n = m if n is None else n
    out = np.zeros(n or 0, dtype=np.int64)
    _lib.check(cond.L.pg_distinct_ids_host(cond.h, _ptr(di), n or 0, None if inn is None else _ptr(inn), ptrs, _ptr(vals), present, _ptr(out)))
    del arrs
    return out


# ---- the value cap: DimensionFieldUniqueFilter, one dimension of GroupWeightCountFilter's size limit ----
DIMCAP_NULL_KEEP, DIMCAP_NULL_VALUE = 0, 1
DIMCAP_CHUNK, DIMCAP_MIN_SLOTS, DIMCAP_LDS_MAX_CAP = 1024, 1024, 6144


def _dimcap_conf(conf):
    """(column, limit, null_mode, null_value | None) → pg_dimcap_conf; the column may be None for the host statement"""
    column, limit, null_mode, null_value = conf
    c = _lib.PgDimcapConf()
    c.column = None if column is None else str(column).encode("utf-8")
    c.limit, c.null_mode = int(limit), int(null_mode)
    c.has_null, c.null_value = (0, 0) if null_value is None else (1, int(null_value))
    return c


def candidates_dimcap_host(conf, keys, rows, score, item_in=None, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """pg_candidates_dimcap_host: the value cap on host arrays by the library's host statement (no context, no device); conf =
    (column | None, limit, DIMCAP_NULL_KEEP | DIMCAP_NULL_VALUE, null_value | None), keys [nq][cap] int64 the entries' values,
    item_in [nq][cap] 0 = the row is outside the store; the rest and the result as Context.candidates_dimcap."""
    nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_dimcap_host", lambda cap: cap, rows, score, source, count, planes_f64,
                                                source_mask, planes_f32)
    k = np.ascontiguousarray(keys, dtype=np.int64)
    inn = None if item_in is None else np.ascontiguousarray(item_in, dtype=np.uint8)
    if k.shape != (nq, cap) or (inn is not None and inn.shape != (nq, cap)):
        raise ValueError("candidates_dimcap_host: keys and item_in are [nq][cap]")
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_candidates_dimcap_host(C.byref(_dimcap_conf(conf)), nq, cap, _ptr(k), v(inn), v(ins[0]), v(ins[1]), v(ins[2]),
                                                     v(ins[3]), v(ins[4]), n64, v(ins[5]), v(ins[6]), n32, *[v(a) for a in outs]))
    return tuple(outs)


class Classcut:
    """A compiled DiversityAdjustCountFilter (pg_classcut_compile): 1..8 classes, each a govaluate boolean expression over declared
    item columns, recall_score and recall_name with a quota.  rules: [(expression, TRIM_FIX | TRIM_ACCUMULATE, count)]; cols:
    [(name, F_I32 | F_I64 | F_F32 | F_F64)]; recall_names: the recalls in fan-in source order.  A host object until a device
    entry first uses it."""

    def __init__(self, rules, cols=(), recall_names=()):
        self.L = _lib.load()
        self.cols = [(str(n), int(d)) for n, d in cols]
        self.recall_names = [str(n) for n in recall_names]
        keep = [str(e).encode("utf-8") for e, _, _ in rules]
        arr = (_lib.PgClasscutRule * max(len(rules), 1))()
        for i, (_, type_, count) in enumerate(rules):
            arr[i] = _lib.PgClasscutRule(keep[i], int(type_), int(count))
        ca = (_lib.PgCondCol * max(len(self.cols), 1))()
        for i, (n, d) in enumerate(self.cols):
            keep.append(n.encode("utf-8"))
            ca[i].name, ca[i].dtype = keep[-1], d
        names = (C.c_char_p * max(len(self.recall_names), 1))(*[n.encode("utf-8") for n in self.recall_names])
        h = C.c_void_p()
        _lib.check(self.L.pg_classcut_compile(arr, len(rules), ca, len(self.cols), names, len(self.recall_names), C.byref(h)))
        del keep
        self.h = h
        self.n_classes = self.L.pg_classcut_num_classes(h)
        self.reads_recall_name = bool(self.L.pg_classcut_reads_recall_name(h))

    def free(self):
        if self.h:
            self.L.pg_classcut_free(self.h)
            self.h = None

    def out_cap(self, cap: int) -> int:
        """pg_classcut_out_cap: min(cap, the FIX counts + the largest ACCUMULATE count).  A host function."""
        out = C.c_uint32()
        _lib.check(self.L.pg_classcut_out_cap(self.h, int(cap), C.byref(out)))
        return out.value

    def _host_cols(self, cols, n):
        """{column name: candidate-aligned values} → (the arrays, kept alive by the caller, and the pointer table)"""
        arrs = []
        ptrs = (C.c_void_p * max(len(self.cols), 1))()
        for i, (name, dt) in enumerate(self.cols):
            if cols is not None and name in cols:
                a = np.ascontiguousarray(cols[name], dtype=_F_NP[dt]).reshape(-1)
                if a.shape[0] != n:
                    raise ValueError("Classcut: column %r holds %d values for %d candidates" % (name, a.shape[0], n))
                arrs.append(a)
                ptrs[i] = a.ctypes.data
        return arrs, ptrs

    def masks_host(self, score, cols=None, item_in=None, source=None) -> np.ndarray:
        """pg_classcut_masks_host: n candidates as candidate-aligned arrays (score [n], {column name: [n]}, item_in [n]: 0 = the
        row is outside the store, source [n]) → [n] uint8, bit c = member of class c."""
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        n = sc.shape[0]
        arrs, ptrs = self._host_cols(cols, n)
        inn = None if item_in is None else np.ascontiguousarray(item_in, dtype=np.uint8).reshape(-1)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8).reshape(-1)
        out = np.zeros(n, dtype=np.uint8)
        _lib.check(self.L.pg_classcut_masks_host(self.h, n, None if inn is None else _ptr(inn), ptrs, None if src is None else _ptr(src),
                                                 _ptr(sc), _ptr(out)))
        del arrs
        return out


def classcut_compile(rules, cols=(), recall_names=()) -> Classcut:
    """pg_classcut_compile (see Classcut)."""
    return Classcut(rules, cols, recall_names)


def classcut_out_cap(cc: Classcut, cap: int) -> int:
    """pg_classcut_out_cap (see Classcut.out_cap): a host function, no context, no device."""
    return cc.out_cap(cap)


def classcut_masks_host(cc: Classcut, score, cols=None, item_in=None, source=None) -> np.ndarray:
    """pg_classcut_masks_host (see Classcut.masks_host): a host function, no context, no device."""
    return cc.masks_host(score, cols, item_in, source)


def candidates_classcut_host(cc: Classcut, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None, cols=None,
                             item_in=None):
    """pg_candidates_classcut_host: DiversityAdjustCountFilter on host arrays by the library's host statement (no context, no
    device); the arrays and the result of Context.candidates_classcut, the columns as candidate-aligned values {name: [nq][cap]}
    and item_in [nq][cap] in place of the store."""
    nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_classcut_host", cc.out_cap, rows, score, source, count, planes_f64, source_mask,
                                                planes_f32)
    arrs, ptrs = cc._host_cols(cols, nq * cap)
    inn = None if item_in is None else np.ascontiguousarray(item_in, dtype=np.uint8).reshape(-1)
    if inn is not None and inn.shape[0] != nq * cap:
        raise ValueError("candidates_classcut_host: item_in is [nq][cap]")
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_candidates_classcut_host(cc.h, nq, cap, v(inn), ptrs, v(ins[0]), v(ins[1]), v(ins[2]), v(ins[3]), v(ins[4]), n64,
                                                       v(ins[5]), v(ins[6]), n32, *[v(a) for a in outs]))
    del arrs
    return tuple(outs)


MIX_FIX, MIX_RANDOM = 1, 2
MIX_MAX_STRATEGIES, MIX_MAX_POSITIONS, MIX_MAX_SIZE = 8, 256, 4096
_MIX_TYPES = {"fix_position": MIX_FIX, "random_position": MIX_RANDOM}


class Mix:
    """A compiled MultiRecallMixSort (pg_mix_compile): 0..8 strategies in config order.  strategies: [MixSortConfig] with the
    reference's JSON keys {MixStrategy: "fix_position" | "random_position" (or MIX_FIX / MIX_RANDOM), Positions, PositionField,
    Number, NumberRate, RecallNames, Conditions: [FilterParamConfig]}; a "SourceMask" key gives the fan-in source bits directly,
    RecallNames are mapped through recall_names (fan-in source order; a name it lacks matches nothing).  cols: [(name, F_*)];
    strings: {value: dictionary id} for string terms.  A host object until a device entry first uses it."""

    def __init__(self, strategies, cols=(), size: int = 0, remain_item: bool = False, recall_names=(), strings: Optional[dict] = None):
        self.L = _lib.load()
        self.cols = [(str(n), int(d)) for n, d in cols]
        self.size, self.remain_item = int(size), bool(remain_item)
        self.strings = dict(strings or {})
        names = [str(n) for n in recall_names]
        keep = []
        arr = (_lib.PgMixStrategy * max(len(strategies), 1))()
        for i, st in enumerate(strategies):
            ty = st.get("MixStrategy", 0)
            arr[i].type = _MIX_TYPES.get(ty, 0) if isinstance(ty, str) else int(ty)
            pos = [int(p) for p in (st.get("Positions") or ())]
            pa = (C.c_int32 * max(len(pos), 1))(*pos)
            keep.append(pa)
            arr[i].positions, arr[i].n_positions = pa, len(pos)
            keep.append(str(st.get("PositionField", "") or "").encode("utf-8"))
            arr[i].position_field = keep[-1]
            arr[i].number = int(st.get("Number", 0) or 0)
            arr[i].number_rate = float(st.get("NumberRate", 0.0) or 0.0)
            mask = int(st.get("SourceMask", 0) or 0)
            for name in st.get("RecallNames") or ():
                if name in names and names.index(name) < 32:
                    mask |= 1 << names.index(name)
            arr[i].source_mask = mask
            terms = _cond_terms(st.get("Conditions", ()) or (), self.strings, keep)
            ta = (_lib.PgCondTerm * max(len(terms), 1))(*terms)
            keep.append(ta)
            arr[i].terms, arr[i].n_terms = ta, len(terms)
        ca = (_lib.PgCondCol * max(len(self.cols), 1))()
        for i, (n, d) in enumerate(self.cols):
            keep.append(n.encode("utf-8"))
            ca[i].name, ca[i].dtype = keep[-1], d
        h = C.c_void_p()
        _lib.check(self.L.pg_mix_compile(arr, len(strategies), ca, len(self.cols), self.size, 1 if self.remain_item else 0, C.byref(h)))
        del keep
        self.h = h
        self.n_strategies = self.L.pg_mix_num_strategies(h)
        self.user_slots = [(self.L.pg_mix_user_slot_name(h, i).decode("utf-8"), bool(self.L.pg_mix_user_slot_is_float(h, i)))
                           for i in range(self.L.pg_mix_num_user_slots(h))]

    def free(self):
        if self.h:
            self.L.pg_mix_free(self.h)
            self.h = None

    pack_user = Cond.pack_user

    def sort_host(self, ctx_size: int, nq: int, cap: int, cols=None, item_in=None, source=None, order=None, count=None, seed=None,
                  users=None):
        """pg_mix_sort_host: the answer on host arrays, no context, no device.  cols {name: [nq][cap]} and item_in [nq][cap] stand
        in for the store (by element); source [nq][cap] u8, order [nq][cap] u32, count [nq] u32, seed [nq] u64, users one
        {name: value} per request → (out_order [nq][cap] u32, out_count [nq] u32)."""
        arrs = []
        ptrs = (C.c_void_p * max(len(self.cols), 1))()
        for i, (name, dt) in enumerate(self.cols):
            if cols is not None and name in cols:
                a = np.ascontiguousarray(cols[name], dtype=_F_NP[dt]).reshape(-1)
                if a.shape[0] != nq * cap:
                    raise ValueError("Mix: column %r holds %d values for %d x %d elements" % (name, a.shape[0], nq, cap))
                arrs.append(a)
                ptrs[i] = a.ctypes.data

        def arr_(a, dt, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
            if a.shape[0] != n:
                raise ValueError("Mix.sort_host: an array holds %d values, %d expected" % (a.shape[0], n))
            return a
        inn, src, ordr = arr_(item_in, np.uint8, nq * cap), arr_(source, np.uint8, nq * cap), arr_(order, np.uint32, nq * cap)
        cnt, sd = arr_(count, np.uint32, nq), arr_(seed, np.uint64, nq)
        uv, up = self.pack_user(users if users is not None else [None] * nq)
        out, oc = np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)
        v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
        _lib.check(self.L.pg_mix_sort_host(self.h, int(ctx_size), nq, cap, v(inn), ptrs, v(src), v(ordr), v(cnt), v(sd), _ptr(uv), _ptr(up),
                                           _ptr(out), _ptr(oc)))
        del arrs
        return out, oc


def mix_compile(strategies, cols=(), size: int = 0, remain_item: bool = False, recall_names=(), strings: Optional[dict] = None) -> Mix:
    """pg_mix_compile (see Mix)."""
    return Mix(strategies, cols, size, remain_item, recall_names, strings)


def mix_sort_host(mix: Mix, ctx_size: int, nq: int, cap: int, **kw):
    """pg_mix_sort_host (see Mix.sort_host): a host function, no context, no device."""
    return mix.sort_host(ctx_size, nq, cap, **kw)


TRAFFIC_PERCENT, TRAFFIC_QUANTITY = 1, 2
TRAFFIC_MAX_TARGETS = 8
_TRAFFIC_TABLES = (500, 1000, 3000, 10000)


def traffic_table(which: int) -> np.ndarray:
    """pg_traffic_table: the whole of table `which` — 0 positionWeight[500], 1 expTable[1000], 2 tanhTable[3000],
    3 sigmoidTable[10000] — as the library built it (float64)."""
    if not 0 <= int(which) < len(_TRAFFIC_TABLES):
        raise ValueError("traffic_table: table %r (0 .. 3)" % (which,))
    out = np.empty(_TRAFFIC_TABLES[int(which)], np.float64)
    _lib.check(_lib.load().pg_traffic_table(int(which), 0, out.shape[0], _ptr(out)))
    return out


class Traffic:
    """A compiled TrafficControlSort target set (pg_traffic_compile): 0..8 targets in config order.  targets: [{TrafficControlTargetId
    (an integer or its decimal string, strconv.Atoi), ControlType: "Percent" (or TRAFFIC_PERCENT) | anything else (TRAFFIC_QUANTITY)}]
    or (target_id, control_type) pairs.  A host object until a device entry first uses it."""

    def __init__(self, targets):
        self.L = _lib.load()
        arr = (_lib.PgTrafficTarget * max(len(targets), 1))()
        for i, t in enumerate(targets):
            if isinstance(t, dict):
                tid, ty = t.get("TrafficControlTargetId", 0), t.get("ControlType", TRAFFIC_QUANTITY)
            else:
                tid, ty = t
            if isinstance(ty, str):
                ty = TRAFFIC_PERCENT if ty == "Percent" else TRAFFIC_QUANTITY
            arr[i].target_id, arr[i].control_type = int(tid), int(ty)
        h = C.c_void_p()
        _lib.check(self.L.pg_traffic_compile(arr, len(targets), C.byref(h)))
        self.h = h
        self.n_targets = self.L.pg_traffic_num_targets(h)

    def free(self):
        if self.h:
            self.L.pg_traffic_free(self.h)
            self.h = None

    def sort_host(self, ctx_size: int, nq: int, cap: int, score=None, member=None, order=None, count=None, alpha=None, page_no: int = 1,
                  gamma: float = 1.0, beta: float = 1.0, eta: float = 1.6, want_control_id: bool = True, want_new_pos: bool = True):
        """pg_traffic_sort_host: the answer on host arrays, no context, no device.  score [nq][cap] f64, member [nq][cap] u8, order
        [nq][cap] u32, count [nq] u32, alpha [nq][T] f64 → (out_order [nq][cap] u32, out_count [nq] u32, control_id [nq][cap] i32
        | None, new_pos [nq][cap] f64 | None)."""
        def arr_(a, dt, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
            if a.shape[0] != n:
                raise ValueError("Traffic.sort_host: an array holds %d values, %d expected" % (a.shape[0], n))
            return a
        sc, mem, ordr = arr_(score, np.float64, nq * cap), arr_(member, np.uint8, nq * cap), arr_(order, np.uint32, nq * cap)
        cnt, al = arr_(count, np.uint32, nq), arr_(alpha, np.float64, nq * self.n_targets)
        out, oc = np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)
        cid = np.empty((nq, cap), np.int32) if want_control_id else None
        pos = np.empty((nq, cap), np.float64) if want_new_pos else None
        v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
        _lib.check(self.L.pg_traffic_sort_host(self.h, int(ctx_size), int(page_no), float(gamma), float(beta), float(eta), nq, cap, v(sc),
                                               v(mem), v(ordr), v(cnt), v(al), _ptr(out), _ptr(oc), v(cid), v(pos)))
        return out, oc, cid, pos


def traffic_compile(targets) -> Traffic:
    """pg_traffic_compile (see Traffic)."""
    return Traffic(targets)


def traffic_sort_host(traffic: Traffic, ctx_size: int, nq: int, cap: int, **kw):
    """pg_traffic_sort_host (see Traffic.sort_host): a host function, no context, no device."""
    return traffic.sort_host(ctx_size, nq, cap, **kw)


def expr_compile_govaluate(source: str) -> "Expr":
    """pg_expr_compile_govaluate: the arithmetic subset of govaluate that BoostScoreSort expressions use."""
    return Expr(source, govaluate=True)


class Context:
    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.L = _lib.load()
        if stream is not None and int(stream) == 0:
            # handle 0 is HIP's null stream (torch's default stream): pg_init reads NULL as "create a private
            # stream", which would silently leave the caller's torch ops and the library's kernels unordered
            raise ValueError("Context: cannot adopt the null stream (handle 0); pass a dedicated stream's handle "
                             "(torch.cuda.Stream().cuda_stream) or None for a private one")
        h = C.c_void_p()
        _lib.check(self.L.pg_init(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        self.stream_handle = int(stream) if stream else None
        self.torch_stream = None

    def close(self):
        if self.h:
            self.L.pg_shutdown(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        _lib.check(self.L.pg_synchronize(self.h))

    def debug_stall(self, ms: int) -> None:
        """Occupy this context's stream for `ms` milliseconds (test aid for the deadline paths)."""
        _lib.check(self.L.pg_debug_stall(self.h, int(ms)))

    def set_option(self, name: str, value) -> None:
        """Developer / test knob of this context (pg_set_option)."""
        _lib.check(self.L.pg_set_option(self.h, name.encode(), str(value).encode()))

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _lib.check(self.L.pg_device_malloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, p: int):
        _lib.check(self.L.pg_device_free(self.h, C.c_void_p(p)))

    def h2d(self, dst: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        _lib.check(self.L.pg_memcpy_h2d(self.h, C.c_void_p(dst), _ptr(a), a.nbytes))

    def d2h(self, a: np.ndarray, src: int):
        assert a.flags.c_contiguous
        _lib.check(self.L.pg_memcpy_d2h(self.h, _ptr(a), C.c_void_p(src), a.nbytes))

    def to_device(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        p = self.malloc(max(a.nbytes, 16))
        self.h2d(p, a)
        return p

    def stats(self) -> _lib.PgStats:
        s = _lib.PgStats()
        _lib.check(self.L.pg_stats(self.h, C.byref(s)))
        return s

    def last_scan_kernel(self) -> Tuple[float, int]:
        ms, b = C.c_double(), C.c_uint64()
        _lib.check(self.L.pg_last_scan_kernel_ms(self.h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    def exclude_compact(self, rows: np.ndarray, scores: np.ndarray, lists, k_out: int, pad_score: float = -np.inf):
        """The compaction kernel alone (pg_exclude_compact_dev): rows / scores [nq][k_in] in a recall's output order and one
        exclusion list of global row ids per request → (rows [nq][k_out], scores [nq][k_out], counts [nq])."""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        nq, k_in = r.shape
        ids, off = _pack_lists(lists, nq)
        if nq and int(np.diff(off.astype(np.int64)).max()) > 4096:       # (the C call cannot check it: its offsets are device memory)
            raise ValueError("exclude_compact: at most 4096 ids per request")
        bufs = [self.to_device(r), self.to_device(sc), self.to_device(ids), self.to_device(off),
                self.malloc(nq * k_out * 8), self.malloc(nq * k_out * 4), self.malloc(nq * 4)]
        try:
            _lib.check(self.L.pg_exclude_compact_dev(self.h, C.c_void_p(bufs[0]), C.c_void_p(bufs[1]), nq, k_in, C.c_void_p(bufs[2]),
                                                     C.c_void_p(bufs[3]), k_out, float(pad_score), C.c_void_p(bufs[4]),
                                                     C.c_void_p(bufs[5]), C.c_void_p(bufs[6])))
            self.synchronize()
            out_r = np.empty((nq, k_out), dtype=np.uint64)
            out_s = np.empty((nq, k_out), dtype=np.float32)
            cnt = np.empty(nq, dtype=np.uint32)
            self.d2h(out_r, bufs[4])
            self.d2h(out_s, bufs[5])
            self.d2h(cnt, bufs[6])
        finally:
            for b in bufs:
                self.free(b)
        return out_r, out_s, cnt

    def fanin_merge_dev(self, sources, nq: int, d_out_rows: int, d_out_score: int, d_out_source: int, d_out_recall_scores: int,
                        d_out_source_mask: int, d_out_count: int) -> None:
        """pg_fanin_merge_dev: sources = [(d_rows, d_scores, k, score_f64)] of device addresses, outputs device addresses
        ([nq][cap] with cap = the sum of the k; d_out_recall_scores [n_sources][nq][cap] and d_out_source_mask may be 0 = not
        wanted).  Enqueued on the context's stream: synchronize() before reading."""
        arr = (_lib.PgFaninSource * max(len(sources), 1))()
        for i, (r, sc, k, f64) in enumerate(sources):
            arr[i] = _lib.PgFaninSource(r or None, sc or None, int(k), int(bool(f64)))
        _lib.check(self.L.pg_fanin_merge_dev(self.h, arr, len(sources), nq, C.c_void_p(d_out_rows or None), C.c_void_p(d_out_score or None),
                                             C.c_void_p(d_out_source or None), C.c_void_p(d_out_recall_scores or None),
                                             C.c_void_p(d_out_source_mask or None), C.c_void_p(d_out_count or None)))

    def fanin_merge(self, sources, recall_scores: bool = True, source_mask: bool = True):
        """Fan-in + UniqueFilter of a request batch's recall answers on host arrays (pg_fanin_merge_dev): sources = [(rows
        [nq][k_s] uint64, scores [nq][k_s] float32 or float64)] in the order the reference would concatenate them →
        (rows [nq][cap] u64, score [nq][cap] f64, source [nq][cap] u8, recall_scores [n][nq][cap] f64 or None,
        source_mask [nq][cap] u32 or None, count [nq] u32)."""
        src = []
        for r, sc in sources:
            r = np.ascontiguousarray(r, dtype=np.uint64)
            sc = np.ascontiguousarray(sc)
            if sc.dtype != np.float64:
                sc = np.ascontiguousarray(sc, dtype=np.float32)
            if r.ndim != 2 or sc.shape != r.shape:
                raise ValueError("fanin_merge: every source is (rows [nq][k], scores [nq][k])")
            src.append((r, sc))
        nq = src[0][0].shape[0] if src else 0
        if any(r.shape[0] != nq for r, _ in src):
            raise ValueError("fanin_merge: every source holds the same requests")
        cap, n = sum(r.shape[1] for r, _ in src), len(src)
        bufs, dev = [], []
        try:
            for r, sc in src:
                bufs += [self.to_device(r), self.to_device(sc)]
                dev.append((bufs[-2], bufs[-1], r.shape[1], sc.dtype == np.float64))
            outs = [np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.float64), np.empty((nq, cap), np.uint8),
                    np.empty((n, nq, cap), np.float64) if recall_scores else None,
                    np.empty((nq, cap), np.uint32) if source_mask else None, np.empty(nq, np.uint32)]
            d_out = []
            for a in outs:
                d_out.append(self.malloc(max(a.nbytes, 16)) if a is not None else 0)
                bufs.append(d_out[-1])
            self.fanin_merge_dev(dev, nq, *d_out)
            self.synchronize()
            for a, p_ in zip(outs, d_out):
                if a is not None and a.nbytes:
                    self.d2h(a, p_)
        finally:
            for b in bufs:
                if b:
                    self.free(b)
        return tuple(outs)

    @staticmethod
    def trim_out_cap(rules, cap: int) -> int:
        """pg_trim_out_cap: the width of what the rules can keep of `cap` entries (validates them; needs no device)."""
        return trim_out_cap(rules, cap)

    def candidates_trim_dev(self, rules, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_planes_f64: int,
                            n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_out_rows: int, d_out_score: int,
                            d_out_source: int, d_out_planes_f64: int, d_out_source_mask: int, d_out_planes_f32: int,
                            d_out_count: int) -> None:
        """pg_candidates_trim_dev: rules = [(source, type, count)], everything else device addresses (0 = absent; an output is
        required exactly where its input is given), outputs [nq][trim_out_cap(rules, cap)].  Enqueued on the context's stream:
        synchronize() before reading."""
        self._list_call(self.L.pg_candidates_trim_dev, (_trim_rules(rules), len(rules)), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count))

    def _list_call(self, fn, lead, nq, cap, lists, before_outputs=()):
        """fn(context, *lead, nq, cap, the ABI's 16 list arguments): `lists` in candidates_trim_dev's order, device addresses (0 =
        absent) but for the two plane counts; before_outputs: addresses an entry takes between the inputs and the outputs"""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        a = [x if i in (5, 8) else v(x) for i, x in enumerate(lists)]
        _lib.check(fn(self.h, *lead, nq, cap, *a[:9], *[v(x) for x in before_outputs], *a[9:]))

    def candidates_trim(self, rules, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
        """Recall quotas / the top-N cut on host arrays (pg_candidates_trim_dev): fanin_merge's rows [nq][cap] u64, score
        [nq][cap] f64, source [nq][cap] u8, count [nq], recall_scores [n][nq][cap] f64 and source_mask, plus planes_f32
        [n][nq][cap] →  (rows, score, source, planes_f64, source_mask, planes_f32, count), [nq][out_cap] each, None where the
        input was None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_trim", lambda cap: trim_out_cap(rules, cap), rows, score, source, count,
                                                    planes_f64, source_mask, planes_f32)
        return self._cand_run(ins, outs, lambda d_in, d_out: self.candidates_trim_dev(
            rules, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, *d_out))

    def _cand_run(self, ins, outs, launch):
        """upload ins, allocate outs, launch(d_in, d_out), synchronise, download, free → outs as a tuple (None stays None and
        travels as address 0; an empty array still gets an allocation, so that it is not taken for an absent one)"""
        bufs = []
        try:
            d_in = []
            for a in ins:
                d_in.append(self.to_device(a) if a is not None and a.nbytes else (self.malloc(16) if a is not None else 0))
                bufs.append(d_in[-1])
            d_out = []
            for a in outs:
                d_out.append(self.malloc(max(a.nbytes, 16)) if a is not None else 0)
                bufs.append(d_out[-1])
            launch(d_in, d_out)
            self.synchronize()
            for a, p_ in zip(outs, d_out):
                if a is not None and a.nbytes:
                    self.d2h(a, p_)
        finally:
            for b in bufs:
                if b:
                    self.free(b)
        return tuple(outs)

    @staticmethod
    def blend_out_cap(conf, cap: int) -> int:
        """pg_blend_out_cap: min(cap, retain_num) (validates the conf; needs no device)."""
        return blend_out_cap(conf, cap)

    def candidates_blend_dev(self, conf, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_planes_f64: int,
                             n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_out_rows: int, d_out_score: int,
                             d_out_source: int, d_out_planes_f64: int, d_out_source_mask: int, d_out_planes_f32: int,
                             d_out_count: int) -> None:
        """pg_candidates_blend_dev: conf = (mode, retain_num, [(source, weight)]), everything else device addresses as
        candidates_trim_dev (0 = absent; an output is required exactly where its input is given), outputs
        [nq][blend_out_cap(conf, cap)].  Enqueued on the context's stream: synchronize() before reading."""
        self._list_call(self.L.pg_candidates_blend_dev, (C.byref(_blend_conf(conf)),), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count))

    def candidates_blend(self, conf, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
        """SnakeFilter / CompletelyFairCountFilter on host arrays (pg_candidates_blend_dev): the arrays of candidates_trim, conf =
        (BLEND_SNAKE_REFILL | BLEND_SNAKE_SKIP | BLEND_FAIR, retain_num, [(source, weight)]) → (rows, score, source, planes_f64,
        source_mask, planes_f32, count), [nq][out_cap] each, None where the input was None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_blend", lambda cap: blend_out_cap(conf, cap), rows, score, source, count,
                                                    planes_f64, source_mask, planes_f32)
        return self._cand_run(ins, outs, lambda d_in, d_out: self.candidates_blend_dev(
            conf, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, *d_out))

    @staticmethod
    def trim2_out_cap(rules, cap: int) -> int:
        """pg_trim2_out_cap: the width of what V2's rules can keep of `cap` entries (validates them; needs no device)."""
        return trim2_out_cap(rules, cap)

    def candidates_trim2_dev(self, rules, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_planes_f64: int,
                             n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_out_rows: int, d_out_score: int,
                             d_out_source: int, d_out_planes_f64: int, d_out_source_mask: int, d_out_planes_f32: int,
                             d_out_count: int) -> None:
        """pg_candidates_trim2_dev: rules = [(source, type, count)], everything else device addresses as candidates_trim_dev (0 =
        absent; an output is required exactly where its input is given), outputs [nq][trim2_out_cap(rules, cap)].  Enqueued on
        the context's stream: synchronize() before reading."""
        self._list_call(self.L.pg_candidates_trim2_dev, (_trim_rules(rules), len(rules)), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count))

    def candidates_trim2(self, rules, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
        """PriorityAdjustCountFilterV2 on host arrays (pg_candidates_trim2_dev): the arrays of candidates_trim, planes_f64 the
        per-recall scores by source index and source_mask the recalls that hold the entry → (rows, score, source, planes_f64,
        source_mask, planes_f32, count), [nq][out_cap] each, None where the input was None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_trim2", lambda cap: trim2_out_cap(rules, cap), rows, score, source, count,
                                                    planes_f64, source_mask, planes_f32)
        return self._cand_run(ins, outs, lambda d_in, d_out: self.candidates_trim2_dev(
            rules, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, *d_out))

    def diversity_rules_dev(self, cfg, n_cols: int, nq: int, cap: int, d_count: int, d_dims: int, d_source: int, d_enable: int,
                            d_order: int) -> None:
        """pg_diversity_rules_dev: device addresses (0 = absent), d_dims [n_cols][nq][cap] int64, d_order [nq][cap] uint32.
        Enqueued on the context's stream: synchronize() before reading."""
        c, keep = _div_config(cfg, n_cols)
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_diversity_rules_dev(self.h, C.byref(c), nq, cap, v(d_count), v(d_dims), v(d_source), v(d_enable), v(d_order)))
        del keep

    def diversity_rules_features_dev(self, cfg, fs, col_names, nq: int, cap: int, d_rows: int, d_count: int, d_source: int,
                                     d_enable: int, d_order: int) -> None:
        """pg_diversity_rules_features_dev: column c of the config is fs's integer column col_names[c] at d_rows [nq][cap] uint64."""
        c, keep = _div_config(cfg, len(col_names))
        names = (C.c_char_p * max(len(col_names), 1))(*[n.encode() for n in col_names])
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_diversity_rules_features_dev(self.h, C.byref(c), getattr(fs, "h", fs), names, nq, cap, v(d_rows), v(d_count),
                                                          v(d_source), v(d_enable), v(d_order)))
        del keep

    def diversity_rules(self, cfg, dims, count=None, source=None, enable=None) -> np.ndarray:
        """DiversityRuleSort of nq requests on host arrays (pg_diversity_rules_dev): dims [n_cols][nq][cap] int64, count [nq],
        source [nq][cap] uint8, enable [nq] bytes → order [nq][cap] uint32 (UINT32_MAX behind count)."""
        d, n_cols, nq, cap, cnt, src, en = _div_planes(dims, count, source, enable)
        return self._cand_run([cnt, d, src, en], [np.empty((nq, cap), np.uint32)], lambda dev, d_out: self.diversity_rules_dev(
            cfg, n_cols, nq, cap, dev[0], dev[1], dev[2], dev[3], d_out[0]))[0]

    def diversity_rules_features(self, cfg, fs, col_names, rows, count=None, source=None, enable=None) -> np.ndarray:
        """The same with the dimension columns read from a feature store (pg_diversity_rules_features_dev): rows [nq][cap] uint64."""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        if r.ndim != 2:
            raise ValueError("diversity_rules_features: rows is [nq][cap]")
        nq, cap = r.shape
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.uint32)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8)
        en = None if enable is None else np.ascontiguousarray(enable, dtype=np.uint8)
        return self._cand_run([r, cnt, src, en], [np.empty((nq, cap), np.uint32)], lambda dev, d_out: self.diversity_rules_features_dev(
            cfg, fs, list(col_names), nq, cap, dev[0], dev[1], dev[2], dev[3], d_out[0]))[0]

    def diversity_rules_one(self, cfg, dims, source=None) -> np.ndarray:
        """pg_diversity_rules: one request on host arrays, dims [n_cols][n] int64 → order [n] uint32 (what the host mirror calls)."""
        d = np.ascontiguousarray(dims, dtype=np.int64)
        if d.ndim != 2:
            raise ValueError("diversity_rules_one: dims is [n_cols][n]")
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8)
        c, keep = _div_config(cfg, d.shape[0])
        out = np.empty(d.shape[1], dtype=np.uint32)
        _lib.check(self.L.pg_diversity_rules(self.h, C.byref(c), d.shape[1], _ptr(d), None if src is None else _ptr(src), _ptr(out)))
        del keep
        return out

    # ---- FilterParam stages: ItemStateFilter, BoostScoreSort ------------------------------------------
    def item_state_filter_dev(self, cond, fs, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int,
                              d_planes_f64: int, n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_user_vals: int,
                              d_user_present: int, d_out_rows: int, d_out_score: int, d_out_source: int, d_out_planes_f64: int,
                              d_out_source_mask: int, d_out_planes_f32: int, d_out_count: int) -> None:
        """pg_item_state_filter_dev: device addresses (0 = absent; an output is required exactly where its input is given),
        outputs [nq][cap].  Enqueued on the context's stream: synchronize() before reading."""
        self._list_call(self.L.pg_item_state_filter_dev, (cond.h, getattr(fs, "h", fs)), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count), (d_user_vals, d_user_present))

    def boost_scores_dev(self, cond, fs, filter_all: bool, nq: int, cap: int, d_rows: int, d_score: int, d_count: int, d_user_vals: int,
                         d_user_present: int, d_out_score: int, d_out_rule: int) -> None:
        """pg_boost_scores_dev: device addresses (0 = absent).  Enqueued on the context's stream: synchronize() before reading."""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_boost_scores_dev(self.h, cond.h, getattr(fs, "h", fs), 1 if filter_all else 0, nq, cap, v(d_rows), v(d_score),
                                              v(d_count), v(d_user_vals), v(d_user_present), v(d_out_score), v(d_out_rule)))

    def _cond_user(self, cond, users, nq):
        if users is None:
            users = [None] * nq
        if len(users) != nq:
            raise ValueError("%d user maps for %d requests" % (len(users), nq))
        return cond.pack_user(users)

    def item_state_filter(self, cond, fs, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None,
                          users=None):
        """ItemStateFilter on host arrays (pg_item_state_filter_dev): fanin_merge's rows [nq][cap] u64, score [nq][cap] f64,
        source [nq][cap] u8, count [nq], planes [n][nq][cap], source_mask [nq][cap] u32; users: one {name: value} per request →
        (rows, score, source, planes_f64, source_mask, planes_f32, count), [nq][cap] each, None where the input was None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("item_state_filter", lambda cap: cap, rows, score, source, count, planes_f64,
                                                    source_mask, planes_f32)
        uv, up = self._cond_user(cond, users, nq)
        return self._cand_run(ins + [uv, up], outs, lambda d_in, d_out: self.item_state_filter_dev(
            cond, fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, d_in[7], d_in[8], *d_out))

    def boost_scores(self, cond, fs, rows, score, count=None, users=None, filter_all: bool = False):
        """BoostScoreSort's rewrite on host arrays (pg_boost_scores_dev): rows [nq][cap] u64, score [nq][cap] f64, count [nq],
        users: one {name: value} per request → (scores [nq][cap] f64, last matching rule [nq][cap] u8, 0xFF = none)."""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        sc = np.ascontiguousarray(score, dtype=np.float64)
        if r.ndim != 2 or sc.shape != r.shape:
            raise ValueError("boost_scores: rows and score are [nq][cap]")
        nq, cap = r.shape
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.uint32)
        uv, up = self._cond_user(cond, users, nq)
        return self._cand_run([r, sc, cnt, uv, up], [np.empty((nq, cap), np.float64), np.empty((nq, cap), np.uint8)],
                              lambda d_in, d_out: self.boost_scores_dev(cond, fs, filter_all, nq, cap, *d_in, *d_out))

    def item_state_filter_one(self, cond, fs, rows, score, source=None, user=None):
        """pg_item_state_filter: one request on host arrays (what the host mirror calls) → (rows [n], score [n], source [n] | None, count)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8).reshape(-1)
        uv, up = cond.pack_user([user])
        o_r, o_s, o_src, cnt = np.empty_like(r), np.empty_like(sc), None if src is None else np.empty_like(src), C.c_uint32()
        _lib.check(self.L.pg_item_state_filter(self.h, cond.h, getattr(fs, "h", fs), r.shape[0], _ptr(r), _ptr(sc),
                                               None if src is None else _ptr(src), _ptr(uv), int(up[0]), _ptr(o_r), _ptr(o_s),
                                               None if src is None else _ptr(o_src), C.byref(cnt)))
        return o_r, o_s, o_src, cnt.value

    def boost_scores_one(self, cond, score, cols=None, item_in=None, user=None, filter_all: bool = False):
        """pg_boost_scores: one request on host arrays, Cond.boost_host's arguments (what the host mirror calls) →
        (scores [n], last matching rule [n])"""
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        m, arrs, ptrs, inn, vals, present = cond._host_args(cols, item_in, user)
        if m is not None and m != sc.shape[0]:
            raise ValueError("boost_scores_one: score and the columns differ in length")
        out, rule = np.empty_like(sc), np.empty(sc.shape[0], dtype=np.uint8)
        _lib.check(self.L.pg_boost_scores(self.h, cond.h, 1 if filter_all else 0, sc.shape[0], None if inn is None else _ptr(inn), ptrs,
                                          _ptr(vals), present, _ptr(sc), _ptr(out), _ptr(rule)))
        del arrs
        return out, rule

    # ---- DistinctIdSort and the value cap (DimensionFieldUniqueFilter) ---------------------------------
    def distinct_ids_dev(self, cond, fs, ids, nq: int, cap: int, d_rows: int, d_count: int, d_user_vals: int, d_user_present: int,
                         d_out_id: int) -> None:
        """pg_distinct_ids_dev: ids a HOST array of one int64 per rule, the rest device addresses (0 = absent), d_out_id [nq][cap]
        int64.  Enqueued on the context's stream: synchronize() before reading."""
        di = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if di.shape[0] != cond.n_rules:
            raise ValueError("distinct_ids_dev: %d ids for %d rules" % (di.shape[0], cond.n_rules))
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_distinct_ids_dev(self.h, cond.h, getattr(fs, "h", fs), _ptr(di), nq, cap, v(d_rows), v(d_count), v(d_user_vals),
                                              v(d_user_present), v(d_out_id)))

    def distinct_ids(self, cond, fs, ids, rows, count=None, users=None) -> np.ndarray:
        """DistinctIdSort's ids on host arrays (pg_distinct_ids_dev): rows [nq][cap] u64, count [nq], users: one {name: value} per
        request → [nq][cap] int64 (the first matching rule's id, else position + 1; padding 0)."""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        if r.ndim != 2:
            raise ValueError("distinct_ids: rows is [nq][cap]")
        nq, cap = r.shape
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.uint32)
        uv, up = self._cond_user(cond, users, nq)
        return self._cand_run([r, cnt, uv, up], [np.empty((nq, cap), np.int64)],
                              lambda d_in, d_out: self.distinct_ids_dev(cond, fs, ids, nq, cap, *d_in, *d_out))[0]

    def distinct_ids_one(self, cond, ids, cols=None, item_in=None, user=None, n: Optional[int] = None) -> np.ndarray:
        """pg_distinct_ids: one request on host arrays, distinct_ids_host's arguments (what the host mirror calls) → [n] int64"""
        di = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if di.shape[0] != cond.n_rules:
            raise ValueError("distinct_ids_one: %d ids for %d rules" % (di.shape[0], cond.n_rules))
        m, arrs, ptrs, inn, vals, present = cond._host_args(cols, item_in, user)
        n = m if n is None else n
        out = np.zeros(n or 0, dtype=np.int64)
        _lib.check(self.L.pg_distinct_ids(self.h, cond.h, _ptr(di), n or 0, None if inn is None else _ptr(inn), ptrs, _ptr(vals), present,
                                          _ptr(out)))
        del arrs
        return out

    def candidates_dimcap_dev(self, conf, fs, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_planes_f64: int,
                              n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_out_rows: int, d_out_score: int,
                              d_out_source: int, d_out_planes_f64: int, d_out_source_mask: int, d_out_planes_f32: int,
                              d_out_count: int) -> None:
        """pg_candidates_dimcap_dev: conf = (column, limit, DIMCAP_NULL_KEEP | DIMCAP_NULL_VALUE, null_value | None), everything
        else device addresses as candidates_trim_dev (0 = absent; an output is required exactly where its input is given),
        outputs [nq][cap].  Enqueued on the context's stream: synchronize() before reading."""
        self._list_call(self.L.pg_candidates_dimcap_dev, (getattr(fs, "h", fs), C.byref(_dimcap_conf(conf))), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count))

    def candidates_dimcap(self, conf, fs, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
        """The value cap on host arrays (pg_candidates_dimcap_dev): the arrays of candidates_trim against the store's column
        conf[0] → (rows, score, source, planes_f64, source_mask, planes_f32, count), [nq][cap] each, None where the input was
        None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_dimcap", lambda cap: cap, rows, score, source, count, planes_f64,
                                                    source_mask, planes_f32)
        return self._cand_run(ins, outs, lambda d_in, d_out: self.candidates_dimcap_dev(
            conf, fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, *d_out))

    def candidates_dimcap_one(self, conf, fs, rows, score, source=None):
        """pg_candidates_dimcap: one request on host arrays (what the host mirror calls) → (rows [n], score [n], source [n] | None, count)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8).reshape(-1)
        o_r, o_s, o_src, cnt = np.empty_like(r), np.empty_like(sc), None if src is None else np.empty_like(src), C.c_uint32()
        _lib.check(self.L.pg_candidates_dimcap(self.h, getattr(fs, "h", fs), C.byref(_dimcap_conf(conf)), r.shape[0], _ptr(r), _ptr(sc),
                                               None if src is None else _ptr(src), _ptr(o_r), _ptr(o_s),
                                               None if src is None else _ptr(o_src), C.byref(cnt)))
        return o_r, o_s, o_src, cnt.value

    # ---- User2ItemExposureBloomFilter -----------------------------------------------------------------------
    def bloom_exists_dev(self, bloom, keys, nq: int, cap: int, d_rows: int, d_count: int, d_slots: int, d_out_exists: int) -> None:
        """pg_bloom_exists_dev: device addresses (d_count 0 = absent), d_out_exists [nq][cap] uint8.  Enqueued on the context's
        stream: synchronize() before reading."""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_bloom_exists_dev(self.h, bloom.h, keys.h, nq, cap, v(d_rows), v(d_count), v(d_slots), v(d_out_exists)))

    def bloom_add_dev(self, bloom, keys, nq: int, cap: int, d_rows: int, d_count: int, d_slots: int) -> None:
        """pg_bloom_add_dev: device addresses (d_count 0 = absent).  Enqueued on the context's stream."""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_bloom_add_dev(self.h, bloom.h, keys.h, nq, cap, v(d_rows), v(d_count), v(d_slots)))

    def bloom_filter_dev(self, bloom, keys, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_planes_f64: int,
                         n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_slots: int, d_out_rows: int, d_out_score: int,
                         d_out_source: int, d_out_planes_f64: int, d_out_source_mask: int, d_out_planes_f32: int, d_out_count: int) -> None:
        """pg_bloom_filter_dev: device addresses as item_state_filter_dev (0 = absent; an output is required exactly where its
        input is given), d_slots [nq] uint32, outputs [nq][cap].  Enqueued on the context's stream: synchronize() before reading."""
        self._list_call(self.L.pg_bloom_filter_dev, (bloom.h, keys.h), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count), (d_slots,))

    @staticmethod
    def _bloom_lists(who, rows, slots, count):
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        if r.ndim != 2:
            raise ValueError("%s: rows is [nq][cap]" % who)
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.uint32)
        if sl.shape != (r.shape[0],) or (cnt is not None and cnt.shape != sl.shape):
            raise ValueError("%s: slots and count are [nq]" % who)
        return r, sl, cnt

    def bloom_exists(self, bloom, keys, rows, slots, count=None) -> np.ndarray:
        """Exists on host arrays (pg_bloom_exists_dev): rows [nq][cap] u64, slots [nq] u32 (BLOOM_NO_SLOT: no history), count [nq]
        → [nq][cap] uint8"""
        r, sl, cnt = self._bloom_lists("bloom_exists", rows, slots, count)
        nq, cap = r.shape
        return self._cand_run([r, cnt, sl], [np.empty((nq, cap), np.uint8)],
                              lambda d_in, d_out: self.bloom_exists_dev(bloom, keys, nq, cap, d_in[0], d_in[1], d_in[2], d_out[0]))[0]

    def bloom_add(self, bloom, keys, rows, slots, count=None) -> None:
        """Add on host arrays (pg_bloom_add_dev), synchronised"""
        r, sl, cnt = self._bloom_lists("bloom_add", rows, slots, count)
        nq, cap = r.shape
        self._cand_run([r, cnt, sl], [], lambda d_in, d_out: self.bloom_add_dev(bloom, keys, nq, cap, d_in[0], d_in[1], d_in[2]))

    def bloom_filter(self, bloom, keys, slots, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
        """The exposure filter on host arrays (pg_bloom_filter_dev): the arrays of candidates_trim, slots [nq] u32 → (rows, score,
        source, planes_f64, source_mask, planes_f32, count), [nq][cap] each, None where the input was None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("bloom_filter", lambda cap: cap, rows, score, source, count, planes_f64, source_mask,
                                                    planes_f32)
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        if sl.shape != (nq,):
            raise ValueError("bloom_filter: slots is [nq]")
        return self._cand_run(ins + [sl], outs, lambda d_in, d_out: self.bloom_filter_dev(
            bloom, keys, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, d_in[7], *d_out))

    def bloom_exists_one(self, bloom, keys, rows, slot: int) -> np.ndarray:
        """pg_bloom_exists: one request on host arrays → [n] uint8"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        out = np.empty(r.shape[0], dtype=np.uint8)
        _lib.check(self.L.pg_bloom_exists(self.h, bloom.h, keys.h, r.shape[0], _ptr(r), int(slot), _ptr(out)))
        return out

    def bloom_add_one(self, bloom, keys, rows, slot: int) -> None:
        """pg_bloom_add: one request on host arrays (logHistory over the returned page)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        _lib.check(self.L.pg_bloom_add(self.h, bloom.h, keys.h, r.shape[0], _ptr(r), int(slot)))

    def bloom_filter_one(self, bloom, keys, rows, score, slot: int, source=None):
        """pg_bloom_filter: one request on host arrays → (rows [n], score [n], source [n] | None, count)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8).reshape(-1)
        o_r, o_s, o_src, cnt = np.empty_like(r), np.empty_like(sc), None if src is None else np.empty_like(src), C.c_uint32()
        _lib.check(self.L.pg_bloom_filter(self.h, bloom.h, keys.h, r.shape[0], _ptr(r), _ptr(sc), None if src is None else _ptr(src), int(slot),
                                          _ptr(o_r), _ptr(o_s), None if src is None else _ptr(o_src), C.byref(cnt)))
        return o_r, o_s, o_src, cnt.value

    # ---- UserGroupHot / GlobalHot / Topic recalls: list recall over a hot table ----------------------------
    def hottable_create(self, table: "Table", n_triggers: int) -> "HotTable":
        """pg_hottable_create: an empty hot table of n_triggers trigger indices over the local rows of `table`"""
        return HotTable(self, table, n_triggers)

    def hottable_upload(self, hot: "HotTable", offsets, item_rows, scores, source, trig0: int = 0) -> None:
        """pg_hottable_upload: append the lists of len(offsets) - 1 consecutive triggers from trig0; trigger trig0 + i lists the
        local rows item_rows[offsets[i]:offsets[i + 1]] with scores[...] (float64) and source[...] (uint8: bits 0-6 the
        RetrieveId index, HOT_UNSCORED = the entry carries no score and its score is 0)"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        it = np.ascontiguousarray(item_rows, dtype=np.uint32)
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        src = np.ascontiguousarray(source, dtype=np.uint8)
        if off.ndim != 1 or off.shape[0] < 1 or it.ndim != 1 or it.shape != sc.shape or it.shape != src.shape or int(off.max()) > it.shape[0]:
            raise ValueError("hottable_upload: offsets must index item_rows / scores / source of one length")
        _lib.check(self.L.pg_hottable_upload(self.h, hot.h, int(trig0), off.shape[0] - 1, _ptr(off), _ptr(it), _ptr(sc), _ptr(src)))

    def hottable_info(self, hot: "HotTable") -> dict:
        rows, nt, pairs, up, gen = C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        _lib.check(self.L.pg_hottable_info(hot.h, C.byref(rows), C.byref(nt), C.byref(pairs), C.byref(up), C.byref(gen)))
        return {"rows": rows.value, "n_triggers": nt.value, "pairs": pairs.value, "triggers_uploaded": up.value, "generation": gen.value}

    def hot_recall_dev(self, hot: "HotTable", mode: int, triggers, k: int, d_out_rows: int, d_out_scores: int, d_out_source: int = 0,
                       d_out_count: int = 0, values=None, d_seed: int = 0) -> None:
        """pg_hot_recall_dev: triggers[q] = request q's trigger indices and values[q] their topic values (HOT_TOPIC only) are host
        lists; d_seed [nq] uint64 (0 = absent) and the outputs [nq][k] / [nq] are device addresses (source and count optional).
        One launch on the context's stream: synchronize() before reading."""
        tr, vals, off = _pack_hot_triggers("hot_recall_dev", mode, triggers, values)
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_hot_recall_dev(self.h, hot.h, int(mode), _ptr(tr), None if vals is None else _ptr(vals), _ptr(off), v(d_seed),
                                            off.shape[0] - 1, int(k), v(d_out_rows), v(d_out_scores), v(d_out_source), v(d_out_count)))

    def hot_recall(self, hot: "HotTable", mode: int, triggers, k: int, values=None, seed=None):
        """pg_hot_recall on host arrays → (rows [nq][k] uint64 global ids, scores [nq][k] f64, source [nq][k] uint8, counts [nq])"""
        tr, vals, off = _pack_hot_triggers("hot_recall", mode, triggers, values)
        nq = off.shape[0] - 1
        sd = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint64).reshape(-1)
        if sd is not None and sd.shape[0] != nq:
            raise ValueError("hot_recall: one seed per request")
        rows, scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
        source, counts = np.empty((nq, k), np.uint8), np.zeros(nq, np.uint32)
        _lib.check(self.L.pg_hot_recall(self.h, hot.h, int(mode), _ptr(tr), None if vals is None else _ptr(vals), _ptr(off),
                                        None if sd is None else _ptr(sd), nq, int(k), _ptr(rows), _ptr(scores), _ptr(source), _ptr(counts)))
        return rows, scores, source, counts

    # ---- DiversityAdjustCountFilter: quotas per expression class ---------------------------------------
    def classcut_masks_dev(self, cc, fs, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_out_masks: int) -> None:
        """pg_classcut_masks_dev: device addresses (0 = absent) → [nq][cap] uint8, bit c = member of class c.  One launch on the
        context's stream: synchronize() before reading."""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_classcut_masks_dev(self.h, cc.h, getattr(fs, "h", fs), nq, cap, v(d_rows), v(d_score), v(d_source), v(d_count),
                                                v(d_out_masks)))

    def classcut_masks(self, cc, fs, rows, score, source=None, count=None) -> np.ndarray:
        """the class masks of host arrays rows / score / source [nq][cap], count [nq] (pg_classcut_masks_dev) → [nq][cap] uint8"""
        nq, cap, ins, _, _, _ = _cand_arrays("classcut_masks", lambda cap: cap, rows, score, source, count, None, None, None)
        out = np.empty((nq, cap), np.uint8)
        return self._cand_run(ins[:4], [out], lambda d_in, d_out: self.classcut_masks_dev(cc, fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3],
                                                                                          d_out[0]))[0]

    def candidates_classcut_dev(self, cc, fs, nq: int, cap: int, d_rows: int, d_score: int, d_source: int, d_count: int, d_planes_f64: int,
                                n_f64: int, d_source_mask: int, d_planes_f32: int, n_f32: int, d_out_rows: int, d_out_score: int,
                                d_out_source: int, d_out_planes_f64: int, d_out_source_mask: int, d_out_planes_f32: int,
                                d_out_count: int) -> None:
        """pg_candidates_classcut_dev: cc a Classcut, fs the store its columns are bound to, everything else device addresses as
        candidates_trim_dev (0 = absent; an output is required exactly where its input is given), outputs [nq][cc.out_cap(cap)].
        Enqueued on the context's stream: synchronize() before reading."""
        self._list_call(self.L.pg_candidates_classcut_dev, (cc.h, getattr(fs, "h", fs)), nq, cap,
                        (d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count))

    def candidates_classcut(self, cc, fs, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
        """DiversityAdjustCountFilter on host arrays (pg_candidates_classcut_dev): the arrays of candidates_trim → (rows, score,
        source, planes_f64, source_mask, planes_f32, count), [nq][out_cap] each, None where the input was None."""
        nq, cap, ins, outs, n64, n32 = _cand_arrays("candidates_classcut", cc.out_cap, rows, score, source, count, planes_f64, source_mask,
                                                    planes_f32)
        return self._cand_run(ins, outs, lambda d_in, d_out: self.candidates_classcut_dev(
            cc, fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, *d_out))

    def candidates_classcut_one(self, cc, fs, rows, score, source=None):
        """pg_candidates_classcut: one request on host arrays (what the host mirror calls) → (rows, score, source | None, count),
        arrays of cc.out_cap(n) entries"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8).reshape(-1)
        w = cc.out_cap(r.shape[0]) if r.shape[0] else 0
        o_r, o_s, o_src, cnt = np.empty(w, np.uint64), np.empty(w, np.float64), None if src is None else np.empty(w, np.uint8), C.c_uint32()
        _lib.check(self.L.pg_candidates_classcut(self.h, cc.h, getattr(fs, "h", fs), r.shape[0], _ptr(r), _ptr(sc),
                                                 None if src is None else _ptr(src), _ptr(o_r), _ptr(o_s),
                                                 None if src is None else _ptr(o_src), C.byref(cnt)))
        return o_r, o_s, o_src, cnt.value

    # ---- MultiRecallMixSort: fixed and random page slots -------------------------------------------------
    def mix_sort_dev(self, mix, fs, ctx_size: int, nq: int, cap: int, d_rows: int, d_source: int, d_order: int, d_count: int, d_seed: int,
                     d_user_vals: int, d_user_present: int, d_out_order: int, d_out_count: int) -> None:
        """pg_mix_sort_dev: device addresses (0 = absent) → d_out_order [nq][cap] u32, d_out_count [nq] u32.  Enqueued on the
        context's stream: synchronize() before reading."""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_mix_sort_dev(self.h, mix.h, getattr(fs, "h", fs), int(ctx_size), nq, cap, v(d_rows), v(d_source), v(d_order),
                                          v(d_count), v(d_seed), v(d_user_vals), v(d_user_present), v(d_out_order), v(d_out_count)))

    def mix_sort(self, mix, fs, ctx_size: int, rows, source=None, order=None, count=None, seed=None, users=None):
        """MultiRecallMixSort on host arrays (pg_mix_sort_dev): rows [nq][cap] u64, source [nq][cap] u8, order [nq][cap] u32 (the
        previous sort's order; None = identity), count [nq], seed [nq] u64, users one {name: value} per request →
        (out_order [nq][cap] u32, out_count [nq] u32)."""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        if r.ndim != 2:
            raise ValueError("mix_sort: rows is [nq][cap]")
        nq, cap = r.shape
        opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)     # noqa: E731
        uv, up = mix.pack_user(users if users is not None else [None] * nq)
        ins = [r, opt(source, np.uint8), opt(order, np.uint32), opt(count, np.uint32), opt(seed, np.uint64), uv, up]
        outs = [np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)]
        return self._cand_run(ins, outs, lambda d_in, d_out: self.mix_sort_dev(mix, fs, ctx_size, nq, cap, *d_in, *d_out))

    def mix_sort_one(self, mix, fs, ctx_size: int, rows, source=None, order=None, seed: int = 0, user=None):
        """pg_mix_sort: one request on host arrays (what the host mirror calls) → (out_order [n] u32, count)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.uint8).reshape(-1)
        ordr = None if order is None else np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
        uv, up = mix.pack_user([user])
        out, cnt = np.empty(r.shape[0], np.uint32), C.c_uint32()
        _lib.check(self.L.pg_mix_sort(self.h, mix.h, getattr(fs, "h", fs), int(ctx_size), r.shape[0], _ptr(r), None if src is None else _ptr(src),
                                      None if ordr is None else _ptr(ordr), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(uv), int(up[0]), _ptr(out),
                                      C.byref(cnt)))
        return out, cnt.value

    # ---- TrafficControlSort: the macro control's re-ranking ----------------------------------------------
    def traffic_sort_dev(self, traffic, ctx_size: int, nq: int, cap: int, d_score: int, d_member: int, d_order: int, d_count: int, d_alpha: int,
                         d_out_order: int, d_out_count: int, d_out_control_id: int = 0, d_out_new_pos: int = 0, page_no: int = 1,
                         gamma: float = 1.0, beta: float = 1.0, eta: float = 1.6) -> None:
        """pg_traffic_sort_dev: device addresses (0 = absent) → d_out_order [nq][cap] u32, d_out_count [nq] u32, d_out_control_id
        [nq][cap] i32, d_out_new_pos [nq][cap] f64.  Enqueued on the context's stream: synchronize() before reading."""
        v = lambda p: C.c_void_p(p or None)                                          # noqa: E731
        _lib.check(self.L.pg_traffic_sort_dev(self.h, traffic.h, int(ctx_size), int(page_no), float(gamma), float(beta), float(eta), nq, cap,
                                              v(d_score), v(d_member), v(d_order), v(d_count), v(d_alpha), v(d_out_order), v(d_out_count),
                                              v(d_out_control_id), v(d_out_new_pos)))

    def traffic_sort(self, traffic, ctx_size: int, score, member, alpha, order=None, count=None, page_no: int = 1, gamma: float = 1.0,
                     beta: float = 1.0, eta: float = 1.6):
        """TrafficControlSort's macro control on host arrays (pg_traffic_sort_dev): score [nq][cap] f64, member [nq][cap] u8, alpha
        [nq][T] f64, order [nq][cap] u32 (None = identity), count [nq] → (out_order [nq][cap] u32, out_count [nq] u32, control_id
        [nq][cap] i32, new_pos [nq][cap] f64)."""
        sc = np.ascontiguousarray(score, dtype=np.float64)
        if sc.ndim != 2:
            raise ValueError("traffic_sort: score is [nq][cap]")
        nq, cap = sc.shape
        opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)     # noqa: E731
        ins = [sc, opt(member, np.uint8), opt(order, np.uint32), opt(count, np.uint32), opt(alpha, np.float64)]
        outs = [np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32), np.empty((nq, cap), np.int32), np.empty((nq, cap), np.float64)]
        return self._cand_run(ins, outs, lambda d_in, d_out: self.traffic_sort_dev(traffic, ctx_size, nq, cap, *d_in, *d_out, page_no=page_no,
                                                                                    gamma=gamma, beta=beta, eta=eta))

    def traffic_sort_one(self, traffic, ctx_size: int, score, member, alpha, order=None, page_no: int = 1, gamma: float = 1.0, beta: float = 1.0,
                         eta: float = 1.6):
        """pg_traffic_sort: one request on host arrays (what the host mirror calls) → (out_order [n] u32, count, control_id [n] i32,
        new_pos [n] f64)"""
        sc = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        mem = np.ascontiguousarray(member, dtype=np.uint8).reshape(-1)
        al = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        ordr = None if order is None else np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
        n = sc.shape[0]
        out, cnt, cid, pos = np.empty(n, np.uint32), C.c_uint32(), np.empty(n, np.int32), np.empty(n, np.float64)
        _lib.check(self.L.pg_traffic_sort(self.h, traffic.h, int(ctx_size), int(page_no), float(gamma), float(beta), float(eta), n, _ptr(sc),
                                          _ptr(mem), None if ordr is None else _ptr(ordr), _ptr(al), _ptr(out), C.byref(cnt), _ptr(cid), _ptr(pos)))
        return out, cnt.value, cid, pos

    # ---- SSDSort: candidate lists in, re-ranked page out ------------------------------------------------
    def ssd_sort_dev(self, table, nq: int, cap: int, d_order, d_rows, d_score, d_source, d_count, d_enable, gamma: float, topn: int,
                     window: int, d_out_pos, d_out_count, d_out_rows=0, d_out_quality=0, normalize_emb: bool = True,
                     ensure_pos_similarity: bool = True, norm_quality_score: int = 0, use_ssd_star: bool = False,
                     candidate_count: int = 0, min_score_percent: float = 0.0, abort_run_cnt: int = 0, filter_source_mask: int = 0):
        """pg_ssd_sort_dev: SSDSort.Sort for nq requests on device arrays.  Every d_* is a torch tensor (anything with
        .data_ptr()) or a raw device address (0 / None = absent): d_order [nq][cap] u32, d_rows [nq][cap] u64, d_score [nq][cap]
        f64, d_source [nq][cap] u8, d_count [nq] u32, d_enable [nq] u8; outputs d_out_pos [nq][cap] u32, d_out_count [nq] u32,
        optional d_out_rows [nq][cap] u64 and d_out_quality [nq][cap] f64 (by input position).  Enqueued on the context's stream:
        synchronize() before reading.  Returns the outputs that were given, (pos, count[, rows][, quality])."""
        def v(p):
            return C.c_void_p((p.data_ptr() if hasattr(p, "data_ptr") else p) or None)
        _lib.check(self.L.pg_ssd_sort_dev(self.h, getattr(table, "h", table), nq, cap, v(d_order), v(d_rows), v(d_score), v(d_source), v(d_count),
                                          v(d_enable), float(gamma), int(topn), int(window), int(normalize_emb), int(ensure_pos_similarity),
                                          int(norm_quality_score), int(use_ssd_star), int(candidate_count), float(min_score_percent),
                                          int(abort_run_cnt), int(filter_source_mask) & 0xFFFFFFFF, v(d_out_pos), v(d_out_count), v(d_out_rows),
                                          v(d_out_quality)))
        absent = lambda p: p is None or (isinstance(p, int) and p == 0)              # noqa: E731
        return tuple(p for p in (d_out_pos, d_out_count, d_out_rows, d_out_quality) if not absent(p))

    # ---- sort / expr (context-level ops) ----------------------------------------------------
    def sort_scores(self, scores: np.ndarray, seg_offsets: Optional[Sequence[int]] = None,
                    descending: bool = True) -> np.ndarray:
        s = np.ascontiguousarray(scores, dtype=np.float64)
        if seg_offsets is None:
            seg_offsets = [0, s.shape[0]]
        so = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        if so.shape[0] < 1 or int(so[-1]) != s.shape[0]:
            # (the C call takes the item count from the last offset: the buffers must be that long)
            raise ValueError("sort_scores: seg_offsets must end at len(scores) = %d" % s.shape[0])
        out = np.zeros(s.shape[0], dtype=np.uint32)
        _lib.check(self.L.pg_sort_scores(self.h, _ptr(s), _ptr(so), so.shape[0] - 1,
                                         int(descending), _ptr(out)))
        return out


class Table:
    """HBM-resident embedding table (module.VectorDao replacement)."""

    def __init__(self, ctx: Context, rows: int, dim: int, row_offset: int = 0):
        self.ctx, self.rows, self.dim, self.row_offset = ctx, rows, dim, row_offset
        h = C.c_void_p()
        _lib.check(ctx.L.pg_table_create(ctx.h, rows, dim, row_offset, C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_table_destroy(self.ctx.h, self.h))
            self.h = None

    def hbm_read_probe(self, reps: int = 3) -> float:
        """Measured streaming-read rate over this table's rows, GB/s."""
        g = C.c_double()
        _lib.check(self.ctx.L.pg_hbm_read_probe(self.ctx.h, self.h, reps, C.byref(g)))
        return g.value

    def screen_info(self) -> Tuple[int, float, float]:
        """(element bytes of the shadow the screened recall streams — 1 int8, 2 bf16, 0 exact fp32 scan —,
        int8 scale, int8 max row residual); builds the shadow if it is not built yet."""
        eb, sc, rs = C.c_int(), C.c_float(), C.c_float()
        _lib.check(self.ctx.L.pg_table_screen_info(self.ctx.h, self.h, C.byref(eb), C.byref(sc), C.byref(rs)))
        return eb.value, sc.value, rs.value

    _DERIVED_DTYPES = {"i8": np.int8, "bf16": np.uint16, "blknorm2": np.float32, "i4": np.uint32, "i4s": np.uint32, "i8r": np.int8,
                       "nx": np.float32, "nxmin": np.float32, "pred": np.uint32}

    def derived_info(self, parts: int = _lib.DERIVED_ALL) -> dict:
        """pg_table_derived_info: builds the asked parts (_lib.DERIVED_*) that are not built yet and returns the scalars of the
        table's derived state as a dict (field names of pg_table_derived_t)."""
        out = _lib.PgTableDerived()
        _lib.check(self.ctx.L.pg_table_derived_info(self.ctx.h, self.h, int(parts), C.byref(out)))
        return {n: getattr(out, n) for n, _ in _lib.PgTableDerived._fields_}

    def derived_len(self, which: str) -> int:
        """elements of one derived array (pg_table_derived_read's layouts)"""
        padded, nblk = self.rows + 64, (self.rows + 31) // 32
        return {"i8": padded * self.dim, "bf16": padded * self.dim, "blknorm2": nblk, "i4": padded * 16, "i4s": padded,
                "i8r": padded * 128, "nx": padded, "nxmin": nblk, "pred": 128 + 128 * 128 + 10}[which]

    def derived_read(self, which: str, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """pg_table_derived_read: elements [first, first + n) of one derived array (a name of _lib.DERIVED_ARRAYS; n = None: to
        the array's end, padding rows included) as a flat numpy array; "pred" comes as uint32 words (f32 mean and covariance,
        then 5 doubles)."""
        if n is None:
            n = self.derived_len(which) - first
        out = np.empty(max(int(n), 0), dtype=self._DERIVED_DTYPES[which])
        _lib.check(self.ctx.L.pg_table_derived_read(self.ctx.h, self.h, _lib.DERIVED_ARRAYS[which], int(first), int(n), _ptr(out)))
        return out

    def fill_synthetic(self, seed: int, normalize: bool = True):
        _lib.check(self.ctx.L.pg_table_fill_synthetic(self.ctx.h, self.h, seed, int(normalize)))

    def fill_gaussian(self, seed: int, sigma: float = 1.0):
        _lib.check(self.ctx.L.pg_table_fill_gaussian(self.ctx.h, self.h, seed, float(sigma)))

    def fill_mixture(self, seed: int, n_centres: int, sigma: float):
        """clustered rows: n_centres centres on the unit sphere, within-cluster noise of norm ~ sigma, normalised"""
        _lib.check(self.ctx.L.pg_table_fill_mixture(self.ctx.h, self.h, seed, int(n_centres), float(sigma)))

    def upload(self, rows: np.ndarray, row0: int = 0):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        assert rows.ndim == 2 and rows.shape[1] == self.dim
        _lib.check(self.ctx.L.pg_table_upload(self.ctx.h, self.h, row0, rows.shape[0], _ptr(rows)))

    def download(self, row0: int, nrows: int) -> np.ndarray:
        out = np.empty((nrows, self.dim), dtype=np.float32)
        _lib.check(self.ctx.L.pg_table_download(self.ctx.h, self.h, row0, nrows, _ptr(out)))
        return out

    def gather(self, rows: Sequence[int]) -> np.ndarray:
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        out = np.empty((r.shape[0], self.dim), dtype=np.float32)
        _lib.check(self.ctx.L.pg_table_gather(self.ctx.h, self.h, _ptr(r), r.shape[0], _ptr(out)))
        return out

    def swap(self, other: "Table"):
        _lib.check(self.ctx.L.pg_table_swap(self.ctx.h, self.h, other.h))
        self.row_offset, other.row_offset = other.row_offset, self.row_offset

    def recall_topk(self, queries: np.ndarray, k: int):
        """queries [nq][dim] → (rows [nq][k] uint64 global ids, scores [nq][k] f32, counts [nq])."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        per_pass = MAX_QUERIES if self.dim <= 128 else 32
        for s in range(0, nq, per_pass):             # one table pass per batch of queries
            e = min(nq, s + per_pass)
            r_, s_, c_ = rows[s:e], scores[s:e], counts[s:e]
            _lib.check(self.ctx.L.pg_recall_topk(self.ctx.h, self.h, _ptr(q[s:e]), e - s, k,
                                                 _ptr(r_), _ptr(s_), _ptr(c_)))
        return rows, scores, counts

    def recall_topk_l2(self, queries: np.ndarray, k: int):
        """HologresVectorRecallV2: queries [nq][dim] → (rows [nq][k], squared Euclidean distances [nq][k] ascending, counts)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.empty((nq, k), dtype=np.uint64)
        dist = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        for s in range(0, nq, MAX_QUERIES):
            e = min(nq, s + MAX_QUERIES)
            r_, d_, c_ = rows[s:e], dist[s:e], counts[s:e]
            _lib.check(self.ctx.L.pg_recall_topk_l2(self.ctx.h, self.h, _ptr(q[s:e]), e - s, k, _ptr(r_), _ptr(d_), _ptr(c_)))
        return rows, dist, counts

    def recall_topk_where(self, feats: "Features", column: str, op: str, value: int, queries: np.ndarray, k: int, l2: bool = False):
        """A Hologres vector recall with its WhereClause `column OP value` (op in > >= < <= == !=): only rows that pass are
        candidates.  → (rows, scores or distances, counts)."""
        ops = {">": 0, ">=": 1, "<": 2, "<=": 3, "==": 4, "!=": 5}
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        col = self.ctx.L.pg_features_column_index(feats.h, column.encode())
        for s in range(0, nq, MAX_QUERIES):
            e = min(nq, s + MAX_QUERIES)
            r_, s_, c_ = rows[s:e], scores[s:e], counts[s:e]
            _lib.check(self.ctx.L.pg_recall_topk_where(self.ctx.h, self.h, feats.h, col, ops[op], int(value), 1 if l2 else 0,
                                                       _ptr(q[s:e]), e - s, k, _ptr(r_), _ptr(s_), _ptr(c_)))
        return rows, scores, counts

    def view(self, feats: "Features", column: str, op: str, value: int) -> "Table":
        """The rows `column OP value` admits, as a table of their own whose recalls answer with THIS table's row ids
        (pg_table_view_create): the WhereClause of a Hologres recall whose constant is fixed when the recall is built."""
        ops = {">": 0, ">=": 1, "<": 2, "<=": 3, "==": 4, "!=": 5}
        col = self.ctx.L.pg_features_column_index(feats.h, column.encode())
        h = C.c_void_p()
        _lib.check(self.ctx.L.pg_table_view_create(self.ctx.h, self.h, feats.h, col, ops[op], int(value), C.byref(h)))
        v = Table.__new__(Table)
        v.ctx, v.dim, v.row_offset, v.h = self.ctx, self.dim, 0, h
        rows = C.c_uint64()
        _lib.check(self.ctx.L.pg_table_info(h, C.byref(rows), None, None))
        v.rows = rows.value
        return v

    def recall_topk_where_ex(self, feats: "Features", where: "Where", queries: np.ndarray, k: int, l2: bool = False):
        """as recall_topk_where with a compiled compound clause (pg_recall_topk_where_ex) → (rows, scores or distances, counts)"""
        return where._recall(self.ctx, self.ctx.L.pg_recall_topk_where_ex, self.h, self.dim, feats, queries, k, l2)

    def view_where(self, feats: "Features", where: "Where") -> "Table":
        """as view with a compiled compound clause (pg_table_view_create_ex)"""
        h = C.c_void_p()
        _lib.check(self.ctx.L.pg_table_view_create_ex(self.ctx.h, self.h, feats.h, where.h, C.byref(h)))
        v = Table.__new__(Table)
        v.ctx, v.dim, v.row_offset, v.h = self.ctx, self.dim, 0, h
        rows = C.c_uint64()
        _lib.check(self.ctx.L.pg_table_info(h, C.byref(rows), None, None))
        v.rows = rows.value
        return v

    def recall_topk_exclude(self, queries: np.ndarray, k: int, lists, l2: bool = False, feats: Optional["Features"] = None,
                            where: Optional["Where"] = None):
        """recall_topk / recall_topk_l2 / recall_topk_where_ex (feats + where) over the rows that are not in the request's
        exclusion list (pg_recall_topk_exclude): lists[q] = the global row ids request q has seen.
        → (rows, scores or distances, counts)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        ids, off = _pack_lists(lists, nq)
        opts = _lib.PgRecallExcludeOpts(1 if l2 else 0, feats.h if feats is not None else None, where.h if where is not None else None)
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_recall_topk_exclude(self.ctx.h, self.h, _ptr(q), nq, k, _ptr(ids), _ptr(off), C.byref(opts),
                                                     _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def i2i_recall(self, trigger_rows, k: int, trigger_table: Optional["Table"] = None, exclude_trigger: bool = False, lists=None):
        """I2IVectorRecall: rows of `trigger_table` (default: this table) are the queries.  exclude_trigger / lists: without
        the trigger item itself / the request's seen items (pg_i2i_recall_exclude)."""
        tr = np.ascontiguousarray(trigger_rows, dtype=np.uint32)
        n = tr.shape[0]
        rows = np.empty((n, k), dtype=np.uint64)
        scores = np.empty((n, k), dtype=np.float32)
        counts = np.zeros(n, dtype=np.uint32)
        if exclude_trigger or lists is not None:
            ids, off = _pack_lists(lists, n)
            _lib.check(self.ctx.L.pg_i2i_recall_exclude(self.ctx.h, (trigger_table or self).h, _ptr(tr), n, self.h, k,
                                                        int(exclude_trigger), _ptr(ids), _ptr(off), _ptr(rows), _ptr(scores),
                                                        _ptr(counts)))
            return rows, scores, counts
        _lib.check(self.ctx.L.pg_i2i_recall(self.ctx.h, (trigger_table or self).h, _ptr(tr), n, self.h, k,
                                            _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def recall_topk_dev(self, d_queries: int, nq: int, k: int, d_out_rows: int, d_out_scores: int):
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_recall_topk_dev(self.ctx.h, self.h, C.c_void_p(d_queries), nq, k,
                                                 C.c_void_p(d_out_rows), C.c_void_p(d_out_scores),
                                                 _ptr(counts)))
        return counts


def _pack_events(rows, codes, play_time, times, now):
    """one list of events per request → (event_rows u32, event_code u16, event_play_time f64 or None, event_time i64,
    offsets u32 [nq + 1], now i64 [nq])"""
    nq = len(rows)
    if len(codes) != nq or len(times) != nq or len(now) != nq or (play_time is not None and len(play_time) != nq):
        raise ValueError("events: every request needs its rows, codes, times and clock")
    er = [np.asarray(a, dtype=np.uint32).reshape(-1) for a in rows]
    ec = [np.asarray(a, dtype=np.uint16).reshape(-1) for a in codes]
    et = [np.asarray(a, dtype=np.int64).reshape(-1) for a in times]
    ep = [np.asarray(a, dtype=np.float64).reshape(-1) for a in play_time] if play_time is not None else None
    if any(a.shape != b.shape or a.shape != c.shape for a, b, c in zip(er, ec, et)) or (ep and any(a.shape != b.shape for a, b in zip(er, ep))):
        raise ValueError("events: every event needs a row, a code and a time")
    off = np.zeros(nq + 1, dtype=np.uint32)
    off[1:] = np.cumsum([a.shape[0] for a in er])

    def cat(arrs, dt):
        return np.ascontiguousarray(np.concatenate(arrs)) if nq else np.zeros(0, dtype=dt)
    return (cat(er, np.uint32), cat(ec, np.uint16), cat(ep, np.float64) if ep is not None else None, cat(et, np.int64), off,
            np.ascontiguousarray(now, dtype=np.int64))


class RtU2I:
    """RealTimeU2IRecall's UserTriggerDaoConf compiled (pg_rtu2i_compile): the trigger-weight expression, the event weights and
    play-time thresholds, the weight mode and the trigger count.  event_names gives events their codes (code = index)."""

    def __init__(self, weight_expression: str, event_names=(), event_weight: str = "", event_play_time: str = "", weight_mode: str = "",
                 trigger_count: int = 0, limit: int = 0):
        names = (C.c_char_p * max(len(event_names), 1))(*[n.encode() for n in event_names])
        conf = _lib.PgRtU2IConf(weight_expression.encode(), event_weight.encode(), event_play_time.encode(), names, len(event_names),
                                weight_mode.encode(), int(trigger_count), int(limit))
        h = C.c_void_p()
        _lib.check(_lib.load().pg_rtu2i_compile(C.byref(conf), C.byref(h)))
        self.h = h
        self.trigger_count = int(_lib.load().pg_rtu2i_trigger_count(h))

    def free(self):
        if self.h:
            _lib.load().pg_rtu2i_free(self.h)
            self.h = None

    def _out(self, nq):
        T = self.trigger_count
        return np.empty((nq, T), dtype=np.uint32), np.empty((nq, T), dtype=np.float64), np.zeros(nq, dtype=np.uint32)

    def triggers_host(self, table_rows: int, rows, codes, play_time, times, now):
        """pg_rtu2i_triggers_host (no context, no device): rows[q], codes[q], play_time[q] (or play_time None), times[q] = request
        q's events, newest first; now[q] its clock → (trigger rows [nq][T] u32, weights [nq][T] f64, counts [nq])"""
        er, ec, ep, et, off, nw = _pack_events(rows, codes, play_time, times, now)
        o = self._out(len(rows))
        _lib.check(_lib.load().pg_rtu2i_triggers_host(self.h, int(table_rows), _ptr(er), _ptr(ec), _ptr(ep) if ep is not None else None, _ptr(et),
                                                     _ptr(off), _ptr(nw), len(rows), _ptr(o[0]), _ptr(o[1]), _ptr(o[2])))
        return o

    def triggers(self, ctx: "Context", table_rows: int, rows, codes, play_time, times, now):
        """pg_rtu2i_triggers: triggers_host's arguments and answer, computed on the device"""
        er, ec, ep, et, off, nw = _pack_events(rows, codes, play_time, times, now)
        o = self._out(len(rows))
        _lib.check(ctx.L.pg_rtu2i_triggers(ctx.h, self.h, int(table_rows), _ptr(er), _ptr(ec), _ptr(ep) if ep is not None else None, _ptr(et),
                                           _ptr(off), _ptr(nw), len(rows), _ptr(o[0]), _ptr(o[1]), _ptr(o[2])))
        return o

    def triggers_dev(self, ctx: "Context", table_rows: int, d_rows: int, d_codes: int, d_play_time: int, d_times: int, offsets, now,
                     d_out_rows: int, d_out_weight: int, d_out_count: int):
        """pg_rtu2i_triggers_dev: events and outputs are device addresses (d_play_time 0: none), offsets and now host arrays"""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        nw = np.ascontiguousarray(now, dtype=np.int64)
        _lib.check(ctx.L.pg_rtu2i_triggers_dev(ctx.h, self.h, int(table_rows), C.c_void_p(d_rows), C.c_void_p(d_codes), d_play_time or None,
                                               C.c_void_p(d_times), _ptr(off), _ptr(nw), off.shape[0] - 1, C.c_void_p(d_out_rows),
                                               C.c_void_p(d_out_weight), C.c_void_p(d_out_count)))


class SimTable:
    """Item-to-item similarity lists over the local rows of `table`, resident in HBM (pg_simtable_*), and the
    collaborative-filter recall over them (pg_cf_recall).  The table must outlive it."""

    def __init__(self, ctx: Context, table: Table):
        self.ctx, self.table = ctx, table
        h = C.c_void_p()
        _lib.check(ctx.L.pg_simtable_create(ctx.h, table.h, C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_simtable_destroy(self.ctx.h, self.h))
            self.h = None

    def info(self) -> dict:
        v = [C.c_uint64() for _ in range(4)]
        _lib.check(self.ctx.L.pg_simtable_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("rows", "pairs", "rows_uploaded", "generation"), (x.value for x in v)))

    def upload(self, offsets, nbr_rows, sims, row0: int = 0):
        """append the lists of len(offsets) - 1 consecutive rows from row0: row row0 + i has the neighbours
        nbr_rows[offsets[i]:offsets[i + 1]] (local rows of the table) with the similarities sims[...]"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        nb = np.ascontiguousarray(nbr_rows, dtype=np.uint32)
        sm = np.ascontiguousarray(sims, dtype=np.float32)
        if off.shape[0] < 1 or nb.shape != sm.shape or nb.ndim != 1 or int(off.max()) > nb.shape[0]:
            raise ValueError("SimTable.upload: offsets must index nbr_rows / sims of one length")
        _lib.check(self.ctx.L.pg_simtable_upload(self.ctx.h, self.h, int(row0), off.shape[0] - 1, _ptr(off), _ptr(nb), _ptr(sm)))

    def cf_recall(self, triggers, prefer, k: int, normalize: bool = True, lists=None):
        """UserCollaborativeFilterRecall: triggers[q] / prefer[q] = request q's trigger rows and preference scores;
        lists[q] = the global row ids request q has seen (None: none).
        → (rows [nq][k] uint64 global ids, scores [nq][k] f64, counts [nq])."""
        nq = len(triggers)
        if len(prefer) != nq:
            raise ValueError("cf_recall: %d preference lists for %d requests" % (len(prefer), nq))
        tr = [np.asarray(t, dtype=np.uint32).reshape(-1) for t in triggers]
        pf = [np.asarray(p, dtype=np.float64).reshape(-1) for p in prefer]
        if any(a.shape != b.shape for a, b in zip(tr, pf)):
            raise ValueError("cf_recall: every trigger needs one preference score")
        off = np.zeros(nq + 1, dtype=np.uint32)
        off[1:] = np.cumsum([a.shape[0] for a in tr])
        trc = np.ascontiguousarray(np.concatenate(tr)) if nq else np.zeros(0, dtype=np.uint32)
        pfc = np.ascontiguousarray(np.concatenate(pf)) if nq else np.zeros(0, dtype=np.float64)
        opts = _lib.PgCfOpts(int(bool(normalize)), None, None)
        if lists is not None:
            ids, xoff = _pack_lists(lists, nq)
            opts.excl_rows, opts.excl_offsets = ids.ctypes.data, xoff.ctypes.data
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_cf_recall(self.ctx.h, self.h, _ptr(trc), _ptr(pfc), _ptr(off), nq, k, C.byref(opts),
                                           _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def cf_recall_dev(self, d_triggers: int, d_prefer: int, trigger_offsets, k: int, d_out_rows: int, d_out_scores: int,
                      normalize: bool = True, d_excl_rows: int = 0, excl_offsets=None):
        """pg_cf_recall_dev: triggers, preferences, lists and outputs are device addresses, the offsets host arrays → counts"""
        off = np.ascontiguousarray(trigger_offsets, dtype=np.uint32)
        nq = off.shape[0] - 1
        opts = _lib.PgCfOpts(int(bool(normalize)), None, None)
        if excl_offsets is not None:
            xoff = np.ascontiguousarray(excl_offsets, dtype=np.uint32)
            opts.excl_rows, opts.excl_offsets = d_excl_rows or None, xoff.ctypes.data
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_cf_recall_dev(self.ctx.h, self.h, C.c_void_p(d_triggers), C.c_void_p(d_prefer), _ptr(off), nq, k,
                                               C.byref(opts), C.c_void_p(d_out_rows), C.c_void_p(d_out_scores), _ptr(counts)))
        return counts

    def rtu2i_expand(self, triggers, prefer, k: int, lists=None):
        """RealTimeU2IRecall's expansion (pg_rtu2i_expand): cf_recall's arguments, but an item keeps the LARGEST of its
        sim * prefer terms and nothing is normalised → (rows [nq][k] uint64 global ids, scores [nq][k] f64, counts [nq])."""
        nq = len(triggers)
        if len(prefer) != nq:
            raise ValueError("rtu2i_expand: %d preference lists for %d requests" % (len(prefer), nq))
        tr = [np.asarray(t, dtype=np.uint32).reshape(-1) for t in triggers]
        pf = [np.asarray(p, dtype=np.float64).reshape(-1) for p in prefer]
        if any(a.shape != b.shape for a, b in zip(tr, pf)):
            raise ValueError("rtu2i_expand: every trigger needs one preference score")
        off = np.zeros(nq + 1, dtype=np.uint32)
        off[1:] = np.cumsum([a.shape[0] for a in tr])
        trc = np.ascontiguousarray(np.concatenate(tr)) if nq else np.zeros(0, dtype=np.uint32)
        pfc = np.ascontiguousarray(np.concatenate(pf)) if nq else np.zeros(0, dtype=np.float64)
        opts = _lib.PgCfOpts(0, None, None)
        if lists is not None:
            ids, xoff = _pack_lists(lists, nq)
            opts.excl_rows, opts.excl_offsets = ids.ctypes.data, xoff.ctypes.data
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_rtu2i_expand(self.ctx.h, self.h, _ptr(trc), _ptr(pfc), _ptr(off), nq, k, C.byref(opts),
                                              _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def rtu2i_expand_dev(self, d_triggers: int, d_prefer: int, trigger_offsets, k: int, d_out_rows: int, d_out_scores: int,
                         d_excl_rows: int = 0, excl_offsets=None):
        """pg_rtu2i_expand_dev: triggers, preferences, lists and outputs are device addresses, the offsets host arrays → counts"""
        off = np.ascontiguousarray(trigger_offsets, dtype=np.uint32)
        nq = off.shape[0] - 1
        opts = _lib.PgCfOpts(0, None, None)
        if excl_offsets is not None:
            xoff = np.ascontiguousarray(excl_offsets, dtype=np.uint32)
            opts.excl_rows, opts.excl_offsets = d_excl_rows or None, xoff.ctypes.data
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_rtu2i_expand_dev(self.ctx.h, self.h, C.c_void_p(d_triggers), C.c_void_p(d_prefer), _ptr(off), nq, k,
                                                  C.byref(opts), C.c_void_p(d_out_rows), C.c_void_p(d_out_scores), _ptr(counts)))
        return counts

    def rtu2i_recall(self, conf: "RtU2I", rows, codes, play_time, times, now, k: int, lists=None):
        """RealTimeU2IRecall (pg_rtu2i_recall): request q's events rows[q], codes[q], play_time[q] (or play_time None), times[q],
        newest first, and its clock now[q] → (rows [nq][k] uint64 global ids, scores [nq][k] f64, counts [nq])."""
        er, ec, ep, et, off, nw = _pack_events(rows, codes, play_time, times, now)
        nq = len(rows)
        opts = _lib.PgCfOpts(0, None, None)
        if lists is not None:
            ids, xoff = _pack_lists(lists, nq)
            opts.excl_rows, opts.excl_offsets = ids.ctypes.data, xoff.ctypes.data
        out_rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_rtu2i_recall(self.ctx.h, conf.h, self.h, _ptr(er), _ptr(ec), _ptr(ep) if ep is not None else None, _ptr(et),
                                              _ptr(off), _ptr(nw), nq, k, C.byref(opts), _ptr(out_rows), _ptr(scores), _ptr(counts)))
        return out_rows, scores, counts

    def rtu2i_recall_dev(self, conf: "RtU2I", d_rows: int, d_codes: int, d_play_time: int, d_times: int, offsets, now, k: int,
                         d_out_rows: int, d_out_scores: int, d_excl_rows: int = 0, excl_offsets=None):
        """pg_rtu2i_recall_dev: events, lists and outputs are device addresses (d_play_time 0: none), offsets and now host
        arrays; enqueue-only between its two kernels → counts"""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        nw = np.ascontiguousarray(now, dtype=np.int64)
        nq = off.shape[0] - 1
        opts = _lib.PgCfOpts(0, None, None)
        if excl_offsets is not None:
            xoff = np.ascontiguousarray(excl_offsets, dtype=np.uint32)
            opts.excl_rows, opts.excl_offsets = d_excl_rows or None, xoff.ctypes.data
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_rtu2i_recall_dev(self.ctx.h, conf.h, self.h, C.c_void_p(d_rows), C.c_void_p(d_codes), d_play_time or None,
                                                  C.c_void_p(d_times), _ptr(off), _ptr(nw), nq, k, C.byref(opts), C.c_void_p(d_out_rows),
                                                  C.c_void_p(d_out_scores), _ptr(counts)))
        return counts


def _pack_triggers(who, triggers, prefer):
    """per-request trigger rows and preference scores → (rows uint32, prefer f64, offsets uint32 [nq + 1])"""
    nq = len(triggers)
    if len(prefer) != nq:
        raise ValueError("%s: %d preference lists for %d requests" % (who, len(prefer), nq))
    tr = [np.asarray(t, dtype=np.uint32).reshape(-1) for t in triggers]
    pf = [np.asarray(p, dtype=np.float64).reshape(-1) for p in prefer]
    if any(a.shape != b.shape for a, b in zip(tr, pf)):
        raise ValueError("%s: every trigger needs one preference score" % who)
    off = np.zeros(nq + 1, dtype=np.uint32)
    off[1:] = np.cumsum([a.shape[0] for a in tr])
    trc = np.ascontiguousarray(np.concatenate(tr)) if nq else np.zeros(0, dtype=np.uint32)
    pfc = np.ascontiguousarray(np.concatenate(pf)) if nq else np.zeros(0, dtype=np.float64)
    return trc, pfc, off


def _x2i_opts(nq, normalize, max_rule, lists):
    """pg_x2i_opts of host lists, and what must stay alive beside it"""
    opts = _lib.PgX2iOpts(int(bool(normalize)), int(bool(max_rule)), None, None)
    keep = None
    if lists is not None:
        keep = _pack_lists(lists, nq)
        opts.excl_rows, opts.excl_offsets = keep[0].ctypes.data, keep[1].ctypes.data
    return opts, keep


def x2i_recall_host(rows: int, row_offset: int, n_x: int, i2x_off, i2x_ids, x2i_off, x2i_rows, x2i_scores, triggers, prefer, k: int,
                    normalize: bool = True, max_rule: bool = False, lists=None):
    """pg_x2i_recall_host: the host statement of the U2I2X2I recall over host CSR arrays (no context, no device)
    → (rows [nq][k] uint64 global ids, scores [nq][k] f64, counts [nq])."""
    nq = len(triggers)
    trc, pfc, off = _pack_triggers("x2i_recall_host", triggers, prefer)
    io = np.ascontiguousarray(i2x_off, dtype=np.uint64)
    ii = np.ascontiguousarray(i2x_ids, dtype=np.uint32)
    xo = np.ascontiguousarray(x2i_off, dtype=np.uint64)
    xr = np.ascontiguousarray(x2i_rows, dtype=np.uint32)
    xs = np.ascontiguousarray(x2i_scores, dtype=np.float32)
    if io.shape[0] != rows + 1 or xo.shape[0] != n_x + 1 or xr.shape != xs.shape or int(io.max()) > ii.shape[0] or int(xo.max()) > xr.shape[0]:
        raise ValueError("x2i_recall_host: the offsets must have rows + 1 / n_x + 1 entries and index their arrays")
    opts, keep = _x2i_opts(nq, normalize, max_rule, lists)
    out_rows = np.empty((nq, k), dtype=np.uint64)
    scores = np.empty((nq, k), dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint32)
    _lib.check(_lib.load().pg_x2i_recall_host(int(rows), int(row_offset), int(n_x), _ptr(io), _ptr(ii), _ptr(xo), _ptr(xr), _ptr(xs), _ptr(trc),
                                              _ptr(pfc), _ptr(off), nq, k, C.byref(opts), _ptr(out_rows), _ptr(scores), _ptr(counts)))
    return out_rows, scores, counts


class XTable:
    """Item -> X and X -> item lists over the local rows of `table` and n_x X values (category, author, tag: the caller's
    dictionary codes), resident in HBM (pg_xtable_*), and the U2I2X2I recall over them (pg_x2i_recall).  The table must outlive it."""

    def __init__(self, ctx: Context, table: Table, n_x: int):
        self.ctx, self.table = ctx, table
        h = C.c_void_p()
        _lib.check(ctx.L.pg_xtable_create(ctx.h, table.h, int(n_x), C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_xtable_destroy(self.ctx.h, self.h))
            self.h = None

    def info(self) -> dict:
        rows, n_x, ip, xp, gen = C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self.ctx.L.pg_xtable_info(self.h, C.byref(rows), C.byref(n_x), C.byref(ip), C.byref(xp), C.byref(gen)))
        return {"rows": rows.value, "n_x": n_x.value, "i2x_pairs": ip.value, "x2i_pairs": xp.value, "generation": gen.value}

    def upload_item2x(self, offsets, x_ids, row0: int = 0):
        """append the X lists of len(offsets) - 1 consecutive rows from row0: row row0 + i has the X x_ids[offsets[i]:offsets[i + 1]]"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(x_ids, dtype=np.uint32)
        if off.shape[0] < 1 or ids.ndim != 1 or int(off.max()) > ids.shape[0]:
            raise ValueError("XTable.upload_item2x: offsets must index x_ids")
        _lib.check(self.ctx.L.pg_xtable_upload_item2x(self.ctx.h, self.h, int(row0), off.shape[0] - 1, _ptr(off), _ptr(ids)))

    def upload_x2item(self, offsets, item_rows, scores, x0: int = 0):
        """append the item lists of len(offsets) - 1 consecutive X from x0: X x0 + i lists the local rows
        item_rows[offsets[i]:offsets[i + 1]] with the scores scores[...] (1.0 where the reference's entry has none)"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        it = np.ascontiguousarray(item_rows, dtype=np.uint32)
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        if off.shape[0] < 1 or it.shape != sc.shape or it.ndim != 1 or int(off.max()) > it.shape[0]:
            raise ValueError("XTable.upload_x2item: offsets must index item_rows / scores of one length")
        _lib.check(self.ctx.L.pg_xtable_upload_x2item(self.ctx.h, self.h, int(x0), off.shape[0] - 1, _ptr(off), _ptr(it), _ptr(sc)))

    def x2i_recall(self, triggers, prefer, k: int, normalize: bool = True, max_rule: bool = False, lists=None):
        """U2I2X2I: triggers[q] / prefer[q] = request q's trigger rows and preference scores; max_rule: the realtime DAO's
        reduction (an item keeps its largest term, nothing normalised); lists[q] = the global row ids request q has seen.
        → (rows [nq][k] uint64 global ids, scores [nq][k] f64, counts [nq]); the outputs of the other requests are
        kept in self.last when a request is beyond a limit (PgError -4)."""
        nq = len(triggers)
        trc, pfc, off = _pack_triggers("x2i_recall", triggers, prefer)
        opts, keep = _x2i_opts(nq, normalize, max_rule, lists)
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint32)
        self.last = (rows, scores, counts)
        _lib.check(self.ctx.L.pg_x2i_recall(self.ctx.h, self.h, _ptr(trc), _ptr(pfc), _ptr(off), nq, k, C.byref(opts),
                                            _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def x2i_recall_dev(self, d_triggers: int, d_prefer: int, trigger_offsets, k: int, d_out_rows: int, d_out_scores: int,
                       normalize: bool = True, max_rule: bool = False, d_excl_rows: int = 0, excl_offsets=None):
        """pg_x2i_recall_dev: triggers, preferences, lists and outputs are device addresses, the offsets host arrays → counts"""
        off = np.ascontiguousarray(trigger_offsets, dtype=np.uint32)
        nq = off.shape[0] - 1
        opts = _lib.PgX2iOpts(int(bool(normalize)), int(bool(max_rule)), None, None)
        if excl_offsets is not None:
            xoff = np.ascontiguousarray(excl_offsets, dtype=np.uint32)
            opts.excl_rows, opts.excl_offsets = d_excl_rows or None, xoff.ctypes.data
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_x2i_recall_dev(self.ctx.h, self.h, C.c_void_p(d_triggers), C.c_void_p(d_prefer), _ptr(off), nq, k,
                                                C.byref(opts), C.c_void_p(d_out_rows), C.c_void_p(d_out_scores), _ptr(counts)))
        return counts

    def rtu2i_x_recall(self, conf: "RtU2I", rows, codes, play_time, times, now, k: int, lists=None):
        """RealTimeU2IRecall over the X table (pg_rtu2i_x_recall): SimTable.rtu2i_recall's events, expanded through the two hops
        with the max rule → (rows [nq][k] uint64 global ids, scores [nq][k] f64, counts [nq])."""
        er, ec, ep, et, off, nw = _pack_events(rows, codes, play_time, times, now)
        nq = len(rows)
        opts, keep = _x2i_opts(nq, False, True, lists)
        out_rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_rtu2i_x_recall(self.ctx.h, conf.h, self.h, _ptr(er), _ptr(ec), _ptr(ep) if ep is not None else None, _ptr(et),
                                                _ptr(off), _ptr(nw), nq, k, C.byref(opts), _ptr(out_rows), _ptr(scores), _ptr(counts)))
        return out_rows, scores, counts

    def rtu2i_x_recall_dev(self, conf: "RtU2I", d_rows: int, d_codes: int, d_play_time: int, d_times: int, offsets, now, k: int,
                           d_out_rows: int, d_out_scores: int, d_excl_rows: int = 0, excl_offsets=None):
        """pg_rtu2i_x_recall_dev: events, lists and outputs are device addresses (d_play_time 0: none), offsets and now host
        arrays; enqueue-only between its two kernels → counts"""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        nw = np.ascontiguousarray(now, dtype=np.int64)
        nq = off.shape[0] - 1
        opts = _lib.PgX2iOpts(0, 1, None, None)
        if excl_offsets is not None:
            xoff = np.ascontiguousarray(excl_offsets, dtype=np.uint32)
            opts.excl_rows, opts.excl_offsets = d_excl_rows or None, xoff.ctypes.data
        counts = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_rtu2i_x_recall_dev(self.ctx.h, conf.h, self.h, C.c_void_p(d_rows), C.c_void_p(d_codes), d_play_time or None,
                                                    C.c_void_p(d_times), _ptr(off), _ptr(nw), nq, k, C.byref(opts), C.c_void_p(d_out_rows),
                                                    C.c_void_p(d_out_scores), _ptr(counts)))
        return counts


HOT_GROUP, HOT_GLOBAL, HOT_TOPIC = 0, 1, 2
HOT_MAX_ENTRIES, HOT_UNSCORED, HOT_PAD_SOURCE = 65536, 0x80, 0xFF


def _pack_hot_triggers(who, mode, triggers, values):
    """per-request trigger indices (and topic values) → (triggers uint32, values f64 | None, offsets uint32 [nq + 1])"""
    nq = len(triggers)
    tr = [np.asarray(t, dtype=np.uint32).reshape(-1) for t in triggers]
    off = np.zeros(nq + 1, dtype=np.uint32)
    off[1:] = np.cumsum([a.shape[0] for a in tr])
    trc = np.ascontiguousarray(np.concatenate(tr)) if nq else np.zeros(0, dtype=np.uint32)
    vals = None
    if values is not None:
        if len(values) != nq:
            raise ValueError("%s: %d value lists for %d requests" % (who, len(values), nq))
        vs = [np.asarray(v, dtype=np.float64).reshape(-1) for v in values]
        if any(a.shape != b.shape for a, b in zip(tr, vs)):
            raise ValueError("%s: every trigger needs one value" % who)
        vals = np.ascontiguousarray(np.concatenate(vs)) if nq else np.zeros(0, dtype=np.float64)
    elif mode == HOT_TOPIC and trc.size:
        raise ValueError("%s: HOT_TOPIC needs the triggers' values" % who)
    if trc.size == 0:                                    # (an address to pass: nothing is read through it)
        trc = np.zeros(1, dtype=np.uint32)
        vals = None if vals is None else np.zeros(1, dtype=np.float64)
    return trc, vals, off


def hot_recall_host(rows: int, row_offset: int, offsets, item_rows, scores, source, mode: int, triggers, k: int, values=None, seed=None):
    """pg_hot_recall_host: the host statement of the list recall over host CSR arrays (no context, no device); offsets
    [n_triggers + 1] → (rows [nq][k] uint64 global ids, scores [nq][k] f64, source [nq][k] uint8, counts [nq])."""
    tr, vals, off = _pack_hot_triggers("hot_recall_host", mode, triggers, values)
    nq = off.shape[0] - 1
    to = np.ascontiguousarray(offsets, dtype=np.uint64)
    it = np.ascontiguousarray(item_rows, dtype=np.uint32)
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    src = np.ascontiguousarray(source, dtype=np.uint8)
    if to.ndim != 1 or to.shape[0] < 2 or it.ndim != 1 or it.shape != sc.shape or it.shape != src.shape or int(to.max()) > it.shape[0]:
        raise ValueError("hot_recall_host: offsets [n_triggers + 1] must index item_rows / scores / source of one length")
    sd = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint64).reshape(-1)
    if sd is not None and sd.shape[0] != nq:
        raise ValueError("hot_recall_host: one seed per request")
    out_rows, out_scores = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float64)
    out_source, counts = np.empty((nq, k), np.uint8), np.zeros(nq, np.uint32)
    _lib.check(_lib.load().pg_hot_recall_host(int(rows), int(row_offset), to.shape[0] - 1, _ptr(to), _ptr(it) if it.size else None,
                                              _ptr(sc) if it.size else None, _ptr(src) if it.size else None, int(mode), _ptr(tr),
                                              None if vals is None else _ptr(vals), _ptr(off), None if sd is None else _ptr(sd), nq, int(k),
                                              _ptr(out_rows), _ptr(out_scores), _ptr(out_source), _ptr(counts)))
    return out_rows, out_scores, out_source, counts


class HotTable:
    """Hot lists over n_triggers trigger indices (trigger ids, topics: the caller's dictionary codes) and the local rows of
    `table`, resident in HBM (pg_hottable_*), for the UserGroupHot / UserGlobalHot / UserTopic recalls (Context.hot_recall).  The
    table must outlive it."""

    def __init__(self, ctx: Context, table: Table, n_triggers: int):
        self.ctx, self.table = ctx, table
        h = C.c_void_p()
        _lib.check(ctx.L.pg_hottable_create(ctx.h, table.h, int(n_triggers), C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_hottable_destroy(self.ctx.h, self.h))
            self.h = None

    def upload(self, offsets, item_rows, scores, source, trig0: int = 0) -> None:
        self.ctx.hottable_upload(self, offsets, item_rows, scores, source, trig0)

    def info(self) -> dict:
        return self.ctx.hottable_info(self)


class Index:
    """Exact IVF-partitioned index over a table (pg_index_*): the same results as the table's own recalls, bit for bit, with
    the lists that provably cannot reach a query's K-th score skipped.  The table must outlive the index."""

    def __init__(self, ctx: Context, table: Table, n_lists: int = 0, train_rows: int = 0, iters: int = 0, seed: int = 0):
        self.ctx, self.table = ctx, table
        p = _lib.PgIndexParams(n_lists, train_rows, iters, seed)
        h = C.c_void_p()
        _lib.check(ctx.L.pg_index_build(ctx.h, table.h, C.byref(p), C.byref(h)))
        self.h = h

    def _recall(self, fn, queries: np.ndarray, k: int):
        dim = self.table.dim
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, dim)
        nq = q.shape[0]
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        per_pass = MAX_QUERIES if dim <= 128 else 32
        for s in range(0, nq, per_pass):             # batches split as Table.recall_topk splits them
            e = min(nq, s + per_pass)
            r_, s_, c_ = rows[s:e], scores[s:e], counts[s:e]
            _lib.check(fn(self.ctx.h, self.h, _ptr(q[s:e]), e - s, k, _ptr(r_), _ptr(s_), _ptr(c_)))
        return rows, scores, counts

    def recall_topk(self, queries: np.ndarray, k: int):
        """as Table.recall_topk → (rows [nq][k] uint64 global ids, scores [nq][k] f32, counts [nq])"""
        return self._recall(self.ctx.L.pg_index_recall_topk, queries, k)

    def recall_topk_l2(self, queries: np.ndarray, k: int):
        """as Table.recall_topk_l2 → (rows, squared Euclidean distances ascending, counts)"""
        return self._recall(self.ctx.L.pg_index_recall_topk_l2, queries, k)

    def recall_topk_dev(self, d_queries: int, nq: int, k: int, d_out_rows: int, d_out_scores: int, l2: bool = False):
        counts = np.zeros(nq, dtype=np.uint32)
        fn = self.ctx.L.pg_index_recall_topk_l2_dev if l2 else self.ctx.L.pg_index_recall_topk_dev
        _lib.check(fn(self.ctx.h, self.h, C.c_void_p(d_queries), nq, k, C.c_void_p(d_out_rows), C.c_void_p(d_out_scores),
                      _ptr(counts)))
        return counts

    def stats(self) -> dict:
        st = _lib.PgIndexStats()
        _lib.check(self.ctx.L.pg_index_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def read(self) -> dict:
        """the build's device arrays (pg_index_read): offsets [n_lists + 1] and perm [rows] uint32, centroids [n_lists][dim],
        cnorm and radius [n_lists] f32"""
        st = self.stats()
        nl, rows, dim = st["n_lists"], st["rows"], st["dim"]
        out = {"offsets": np.empty(nl + 1, np.uint32), "perm": np.empty(rows, np.uint32),
               "centroids": np.empty((nl, dim), np.float32), "cnorm": np.empty(nl, np.float32), "radius": np.empty(nl, np.float32)}
        _lib.check(self.ctx.L.pg_index_read(self.ctx.h, self.h, *(_ptr(out[n]) for n in ("offsets", "perm", "centroids", "cnorm",
                                                                                          "radius"))))
        return out

    def bounds(self, queries: np.ndarray, l2: bool = False) -> np.ndarray:
        """U [nq][n_lists] f32 as the search computes it (pg_index_bounds): >= every chain score of a list's rows (l2: of -d)"""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.table.dim)
        out = np.empty((q.shape[0], self.stats()["n_lists"]), np.float32)
        _lib.check(self.ctx.L.pg_index_bounds(self.ctx.h, self.h, _ptr(q), q.shape[0], int(l2), _ptr(out)))
        return out

    def recall_topk_where(self, feats: "Features", column: str, op: str, value: int, queries: np.ndarray, k: int, l2: bool = False):
        """as Table.recall_topk_where, through the index over the filter's lists (pg_index_recall_topk_where)
        → (rows, scores or distances, counts)"""
        ops = {">": 0, ">=": 1, "<": 2, "<=": 3, "==": 4, "!=": 5}
        dim = self.table.dim
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, dim)
        nq = q.shape[0]
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        col = self.ctx.L.pg_features_column_index(feats.h, column.encode())
        for s in range(0, nq, MAX_QUERIES):          # batches split as Table.recall_topk_where splits them
            e = min(nq, s + MAX_QUERIES)
            r_, s_, c_ = rows[s:e], scores[s:e], counts[s:e]
            _lib.check(self.ctx.L.pg_index_recall_topk_where(self.ctx.h, self.h, feats.h, col, ops[op], int(value), 1 if l2 else 0,
                                                             _ptr(q[s:e]), e - s, k, _ptr(r_), _ptr(s_), _ptr(c_)))
        return rows, scores, counts

    def recall_topk_where_ex(self, feats: "Features", where: "Where", queries: np.ndarray, k: int, l2: bool = False):
        """as Table.recall_topk_where_ex, through the index over the clause's lists (pg_index_recall_topk_where_ex)"""
        return where._recall(self.ctx, self.ctx.L.pg_index_recall_topk_where_ex, self.h, self.table.dim, feats, queries, k, l2)

    def where_read(self, feats: "Features", column: str, op: str, value: int) -> dict:
        """a filter's lists over the index (pg_index_where_read, built or from the cache): offsets [n_lists + 1] and perm
        [admitted] uint32 — list L holds perm[offsets[L]:offsets[L + 1]], the index's rows of L that pass, in order"""
        ops = {">": 0, ">=": 1, "<": 2, "<=": 3, "==": 4, "!=": 5}
        st = self.stats()
        col = self.ctx.L.pg_features_column_index(feats.h, column.encode())
        offsets = np.empty(st["n_lists"] + 1, np.uint32)
        perm = np.empty(max(st["rows"], 1), np.uint32)
        admitted = C.c_uint64()
        _lib.check(self.ctx.L.pg_index_where_read(self.ctx.h, self.h, feats.h, col, ops[op], int(value), _ptr(offsets), _ptr(perm),
                                                  C.byref(admitted)))
        return {"offsets": offsets, "perm": perm[:admitted.value].copy(), "admitted": admitted.value}

    def where_stats(self) -> dict:
        """the filtered lists' cache: builds, hits, evictions, entries held and their device bytes (pg_index_where_stats)"""
        st = _lib.PgIndexWhereStats()
        _lib.check(self.ctx.L.pg_index_where_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def refresh(self, mode: str = "auto", force: bool = False, ctx: Context = None):
        """Bring the index back to the table's current rows, keeping its centroids (pg_index_refresh): "incremental" re-assigns
        the rows the table's write log holds, "full" every row (on the matrix pipe), "auto" picks; a current index is left
        alone unless force.  Results stay bit for bit the table's."""
        p = _lib.PgIndexRefreshParams({"auto": 0, "full": 1, "incremental": 2}[mode], int(force))
        _lib.check(self.ctx.L.pg_index_refresh((ctx or self.ctx).h, self.h, C.byref(p)))

    def refresh_stats(self) -> dict:
        """refreshes by kind, rows re-assigned / moved / sent to the fp32 kernel, the generation described, the last refresh's
        wall and assignment times (pg_index_refresh_stats)"""
        st = _lib.PgIndexRefreshStats()
        _lib.check(self.ctx.L.pg_index_refresh_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def attach(self, ctx: Context = None):
        """Route every recall job of the table (plain recalls, coalescer batches, recommend pipelines) through this index first
        (pg_index_attach); a second attached index replaces the first."""
        _lib.check(self.ctx.L.pg_index_attach((ctx or self.ctx).h, self.h))

    def detach(self, ctx: Context = None):
        """Stop routing the table's recalls through this index; returns once nothing enqueued reads it (pg_index_detach)."""
        _lib.check(self.ctx.L.pg_index_detach((ctx or self.ctx).h, self.h))

    def serving_stats(self) -> dict:
        """plans tried / held, re-plans by reason and skipped batches of the attached plan (pg_index_serving_stats)"""
        st = _lib.PgIndexServingStats()
        _lib.check(self.ctx.L.pg_index_serving_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_index_destroy(self.ctx.h, self.h))
            self.h = None


def index_screen_probe(ctx: Context, rows: np.ndarray, centroids: np.ndarray):
    """the matrix-pipe screen of Index.refresh's full mode on host rows and centroids (pg_index_screen_probe)
    → (s [n][n_lists] the screen's distances, e [n][n_lists] its bound; +inf outside the range the bound is claimed for)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    cent = np.ascontiguousarray(centroids, dtype=np.float32).reshape(-1, rows.shape[1])
    s = np.empty((rows.shape[0], cent.shape[0]), np.float32)
    e = np.empty_like(s)
    _lib.check(ctx.L.pg_index_screen_probe(ctx.h, rows.shape[1], _ptr(rows), rows.shape[0], _ptr(cent), cent.shape[0], _ptr(s),
                                           _ptr(e)))
    return s, e


def pack_dnn3(w1, b1, w2, b2, w3, b3, d_user: int) -> bytes:
    w1 = np.ascontiguousarray(w1, dtype=np.float32)
    w2 = np.ascontiguousarray(w2, dtype=np.float32)
    din, h1 = w1.shape
    h2 = w2.shape[1]
    return (struct.pack("<4I", d_user, din - d_user, h1, h2) + w1.tobytes() +
            np.ascontiguousarray(b1, dtype=np.float32).tobytes() + w2.tobytes() +
            np.ascontiguousarray(b2, dtype=np.float32).tobytes() +
            np.ascontiguousarray(w3, dtype=np.float32).tobytes() + struct.pack("<f", float(b3)))


def pack_dnn3_multi(w1, b1, w2, b2, w3, b3, d_user: int) -> bytes:
    """PG_MODEL_DNN3_MULTI blob (include/pairec_gpu.h): w3 [h2][n_out], b3 [n_out] — n_out heads on one trunk."""
    w1 = np.ascontiguousarray(w1, dtype=np.float32)
    w2 = np.ascontiguousarray(w2, dtype=np.float32)
    w3 = np.ascontiguousarray(w3, dtype=np.float32)
    b3 = np.ascontiguousarray(b3, dtype=np.float32).reshape(-1)
    din, h1 = w1.shape
    h2 = w2.shape[1]
    assert w3.shape == (h2, b3.shape[0])
    return (struct.pack("<5I", d_user, din - d_user, h1, h2, b3.shape[0]) + w1.tobytes() +
            np.ascontiguousarray(b1, dtype=np.float32).tobytes() + w2.tobytes() +
            np.ascontiguousarray(b2, dtype=np.float32).tobytes() + w3.tobytes() + b3.tobytes())


def pack_fm2t(w) -> bytes:
    """w: object with the attributes of oracle.Fm2tWeights (duck-typed; no oracle import here)."""
    parts = [struct.pack("<7If", w.nuf, w.nif, w.k, w.d_user, w.t_h1, w.t_out, w.vocab, w.fm_b)]
    for a in (w.uw1, w.ub1, w.uw2, w.ub2, w.iw1, w.ib1, w.iw2, w.ib2):
        parts.append(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    for f in range(w.nuf + w.nif):
        parts.append(np.ascontiguousarray(w.field_emb[f], dtype=np.float32).tobytes())
        parts.append(np.ascontiguousarray(w.field_lin[f], dtype=np.float32).tobytes())
    return b"".join(parts)


class RankModel:
    """Rank model resident in HBM (algorithm/eas | tfserving predict replacement)."""

    def __init__(self, ctx: Context, kind: int, prec: int, blob: bytes):
        self.ctx, self.kind, self.prec = ctx, kind, prec
        self._blob_head = bytes(blob[:28])
        h = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        _lib.check(ctx.L.pg_model_load(ctx.h, kind, prec, buf, len(blob), C.byref(h)))
        self.h = h
        n = C.c_uint32()
        _lib.check(ctx.L.pg_model_num_outputs(h, C.byref(n)))
        self.n_out = n.value

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_model_destroy(self.ctx.h, self.h))
            self.h = None

    def f16_stats(self) -> dict:
        """PREC_F16X2 / PREC_F16: how much of the model's work the fp16 kernel took and how much went back to BF16X3
        (waits for the context to drain)."""
        out = (C.c_uint64 * 4)()
        _lib.check(self.ctx.L.pg_model_f16_stats(self.h, out))
        return {"calls": int(out[0]), "tiles": int(out[1]), "tiles_served_bf16x3": int(out[2]),
                "calls_served_bf16x3_whole": int(out[3])}

    def rank_dnn3(self, table: Table, user_vecs: np.ndarray, cand_rows: np.ndarray,
                  req_offsets: Sequence[int]) -> np.ndarray:
        """scores [n_items]; a multi-output model: [n_out][n_items] (one plane per head)."""
        u = np.ascontiguousarray(user_vecs, dtype=np.float32)
        c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        ro = np.ascontiguousarray(req_offsets, dtype=np.uint32)
        out = np.empty((self.n_out, c.shape[0]), dtype=np.float32)
        _lib.check(self.ctx.L.pg_rank_dnn3(self.ctx.h, self.h, table.h, _ptr(u), _ptr(c), _ptr(ro),
                                           ro.shape[0] - 1, _ptr(out)))
        return out[0] if self.n_out == 1 else out

    def rank_dnn3_dev(self, table: Table, d_user_vecs: int, d_cand_rows: int, d_req_offsets: int,
                      n_req: int, n_items: int, d_out: int):
        _lib.check(self.ctx.L.pg_rank_dnn3_dev(self.ctx.h, self.h, table.h, C.c_void_p(d_user_vecs),
                                               C.c_void_p(d_cand_rows), C.c_void_p(d_req_offsets),
                                               n_req, n_items, C.c_void_p(d_out)))

    def rank_fm2t(self, user_vecs, user_field_ids, item_field_ids, req_offsets) -> np.ndarray:
        u = np.ascontiguousarray(user_vecs, dtype=np.float32)
        uf = np.ascontiguousarray(user_field_ids, dtype=np.int32)
        itf = np.ascontiguousarray(item_field_ids, dtype=np.int32)
        ro = np.ascontiguousarray(req_offsets, dtype=np.uint32)
        out = np.empty(int(ro[-1]), dtype=np.float32)
        _lib.check(self.ctx.L.pg_rank_fm2t(self.ctx.h, self.h, _ptr(u), _ptr(uf), _ptr(itf),
                                           _ptr(ro), ro.shape[0] - 1, _ptr(out)))
        return out


    def user_embedding(self, user_vecs: np.ndarray) -> np.ndarray:
        """Two-tower user embedding [n][t_out] (pg_fm2t_user_embedding)."""
        u = np.ascontiguousarray(user_vecs, dtype=np.float32)
        u = u.reshape(-1, u.shape[-1])
        hdr = struct.unpack("<7I", self._blob_head)
        out = np.empty((u.shape[0], hdr[5]), dtype=np.float32)
        _lib.check(self.ctx.L.pg_fm2t_user_embedding(self.ctx.h, self.h, _ptr(u), u.shape[0], _ptr(out)))
        return out

    def online_vector_recall(self, item_emb: Table, user_vecs: np.ndarray, k: int):
        """OnlineVectorRecall: user tower → top-k of the item-embedding table."""
        u = np.ascontiguousarray(user_vecs, dtype=np.float32)
        u = u.reshape(-1, u.shape[-1])
        n = u.shape[0]
        rows = np.empty((n, k), dtype=np.uint64)
        scores = np.empty((n, k), dtype=np.float32)
        counts = np.zeros(n, dtype=np.uint32)
        _lib.check(self.ctx.L.pg_online_vector_recall(self.ctx.h, self.h, item_emb.h, _ptr(u), n, k, _ptr(rows),
                                                      _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def rank_fm2t_rows(self, feats: "Features", item_field_names, user_vecs, user_field_ids, cand_rows,
                       req_offsets) -> np.ndarray:
        """FM + two-tower rank from candidate rows: the item field ids come from feature columns."""
        ctx = self.ctx
        u = np.ascontiguousarray(user_vecs, dtype=np.float32)
        uf = np.ascontiguousarray(user_field_ids, dtype=np.int32)
        cr = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        ro = np.ascontiguousarray(req_offsets, dtype=np.uint32)
        cols = feats._cols(item_field_names)
        n = int(ro[-1])
        d_u, d_uf, d_cr, d_ro = ctx.to_device(u), ctx.to_device(uf), ctx.to_device(cr), ctx.to_device(ro)
        d_o = ctx.malloc(max(n * 4, 16))
        _lib.check(ctx.L.pg_rank_fm2t_rows_dev(ctx.h, self.h, feats.h, _ptr(cols), d_u, d_uf, d_cr, d_ro,
                                               ro.shape[0] - 1, n, d_o))
        out = np.zeros(n, dtype=np.float32)
        ctx.d2h(out, d_o)
        for p in (d_u, d_uf, d_cr, d_ro, d_o):
            ctx.free(p)
        return out


class ItemRows:
    """Materialised item records of an FM + two-tower model (pg_fm2t_item_rows_*): one contiguous 640-B record per
    item row, built once from the model's field tables and the item-field columns."""

    def __init__(self, model: "RankModel", feats: "Features", item_field_names):
        self.ctx, self.model, self.feats = model.ctx, model, feats
        cols = feats._cols(item_field_names)
        h = C.c_void_p()
        _lib.check(self.ctx.L.pg_fm2t_item_rows_build(self.ctx.h, model.h, feats.h, _ptr(cols), C.byref(h)))
        self.h = h

    def update(self, row0: int, nrows: int):
        _lib.check(self.ctx.L.pg_fm2t_item_rows_update(self.ctx.h, self.h, row0, nrows))

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_fm2t_item_rows_destroy(self.ctx.h, self.h))
            self.h = None

    def rank(self, user_vecs, user_field_ids, cand_rows, req_offsets) -> np.ndarray:
        """pg_rank_fm2t_irows (host buffers)."""
        u = np.ascontiguousarray(user_vecs, dtype=np.float32)
        uf = np.ascontiguousarray(user_field_ids, dtype=np.int32)
        cr = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        ro = np.ascontiguousarray(req_offsets, dtype=np.uint32)
        out = np.empty(int(ro[-1]), dtype=np.float32)
        _lib.check(self.ctx.L.pg_rank_fm2t_irows(self.ctx.h, self.model.h, self.h, _ptr(u), _ptr(uf), _ptr(cr), _ptr(ro),
                                                 ro.shape[0] - 1, _ptr(out)))
        return out


def rank_fm2t_rows_host(model: "RankModel", feats: "Features", item_field_names, user_vecs, user_field_ids, cand_rows,
                        req_offsets) -> np.ndarray:
    """pg_rank_fm2t_rows: the host-buffer form (what a caller-made batch of IAlgorithm.Run calls passes)."""
    ctx = model.ctx
    u = np.ascontiguousarray(user_vecs, dtype=np.float32)
    uf = np.ascontiguousarray(user_field_ids, dtype=np.int32)
    cr = np.ascontiguousarray(cand_rows, dtype=np.uint32)
    ro = np.ascontiguousarray(req_offsets, dtype=np.uint32)
    cols = feats._cols(item_field_names)
    out = np.empty(int(ro[-1]), dtype=np.float32)
    _lib.check(ctx.L.pg_rank_fm2t_rows(ctx.h, model.h, feats.h, _ptr(cols), _ptr(u), _ptr(uf), _ptr(cr), _ptr(ro),
                                       ro.shape[0] - 1, _ptr(out)))
    return out


class Where:
    """A compiled compound WhereClause (pg_where_*): AND / OR / NOT / IN / BETWEEN over the integer columns of a Features store.
    Compiling needs no GPU; the columns are resolved by name at each use."""

    def __init__(self, clause: str):
        self.L = _lib.load()
        h = C.c_void_p()
        _lib.check(self.L.pg_where_compile(clause.encode("utf-8"), C.byref(h)))
        self.h = h
        self.columns = [self.L.pg_where_column_name(h, i).decode("utf-8") for i in range(self.L.pg_where_num_columns(h))]

    def free(self):
        if self.h:
            self.L.pg_where_free(self.h)
            self.h = None

    def eval_host(self, cols: dict, rows: Optional[int] = None) -> np.ndarray:
        """cols: {column name: int32 or int64 array} → the bitmap [(rows + 31) // 32] uint32 (pg_where_eval_host): bit r & 31 of
        word r >> 5 is set when row r passes"""
        arrs = []
        for n in self.columns:
            a = np.asarray(cols[n])
            if a.dtype not in (np.int32, np.int64):
                raise TypeError("Where.eval_host: column %r is %s, not int32 / int64" % (n, a.dtype))
            arrs.append(np.ascontiguousarray(a))
        if rows is None:
            rows = arrs[0].shape[0]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        dts = (C.c_int * max(len(arrs), 1))(*[F_I64 if a.dtype == np.int64 else F_I32 for a in arrs])
        out = np.zeros((rows + 31) // 32, dtype=np.uint32)
        _lib.check(self.L.pg_where_eval_host(self.h, ptrs, dts, rows, _ptr(out)))
        return out

    def bits(self, ctx: "Context", feats: "Features", rows: int):
        """the device's bitmap for `rows` rows of `feats`, built or from the cache (pg_where_bits) → (bitmap uint32, admitted)"""
        out = np.zeros((rows + 31) // 32, dtype=np.uint32)
        n = C.c_uint64()
        _lib.check(self.L.pg_where_bits(ctx.h, self.h, feats.h, rows, _ptr(out), C.byref(n)))
        return out, n.value

    def stats(self) -> dict:
        st = _lib.PgWhereStats()
        _lib.check(self.L.pg_where_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def _recall(self, ctx, fn, over, dim: int, feats: "Features", queries: np.ndarray, k: int, l2: bool):
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, dim)
        nq = q.shape[0]
        rows = np.empty((nq, k), dtype=np.uint64)
        scores = np.empty((nq, k), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        for s in range(0, nq, MAX_QUERIES):          # batches split as Table.recall_topk_where splits them
            e = min(nq, s + MAX_QUERIES)
            r_, s_, c_ = rows[s:e], scores[s:e], counts[s:e]
            _lib.check(fn(ctx.h, over, feats.h, self.h, 1 if l2 else 0, _ptr(q[s:e]), e - s, k, _ptr(r_), _ptr(s_), _ptr(c_)))
        return rows, scores, counts


BLOOM_MAX_KEY, BLOOM_MAX_K, BLOOM_NO_SLOT = 64, 16, 0xFFFFFFFF


def bloom_estimate(n: int, p: float) -> Tuple[int, int]:
    """pg_bloom_estimate: EstimateParameters (bloom.go:40-45) → (m, k).  A host function: no context, no device."""
    m, k = C.c_uint64(), C.c_uint32()
    _lib.check(_lib.load().pg_bloom_estimate(int(n), float(p), C.byref(m), C.byref(k)))
    return m.value, k.value


def bloom_murmur3_host(data: bytes, seed: int = 0) -> int:
    """pg_bloom_murmur3_host: murmur3_x86_32 of the bytes with a seed."""
    out = C.c_uint32()
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    _lib.check(_lib.load().pg_bloom_murmur3_host(_ptr(a) if a.size else None, a.size, int(seed) & 0xFFFFFFFF, C.byref(out)))
    return out.value


def bloom_pack_keys(keys):
    """a sequence of bytes objects → (offsets uint64 [rows + 1], bytes uint8): what pg_bloom_keys_create and the host statements take"""
    off = np.zeros(len(keys) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    return off, np.frombuffer(b"".join(bytes(k) for k in keys), dtype=np.uint8).copy()


def _bloom_host_args(who, m, k, seeds, bitsets, key_offsets, key_bytes, rows, count, slots):
    bs = np.ascontiguousarray(bitsets, dtype=np.uint8)
    if bs.ndim != 2:
        raise ValueError("%s: bitsets is [n_slots][ceil(m / 8)] bytes" % who)
    sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
    if sd is not None and sd.shape != (k,):
        raise ValueError("%s: one seed per hash" % who)
    ko, kb = np.ascontiguousarray(key_offsets, dtype=np.uint64), np.ascontiguousarray(key_bytes, dtype=np.uint8)
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    if r.ndim != 2:
        raise ValueError("%s: rows is [nq][cap]" % who)
    cnt = None if count is None else np.ascontiguousarray(count, dtype=np.uint32)
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    if sl.shape != (r.shape[0],) or (cnt is not None and cnt.shape != sl.shape):
        raise ValueError("%s: slots and count are [nq]" % who)
    return bs, sd, ko, kb, r, cnt, sl


def bloom_exists_host(m: int, k: int, seeds, bitsets, key_offsets, key_bytes, rows, slots, count=None) -> np.ndarray:
    """pg_bloom_exists_host: bitsets [n_slots][ceil(m / 8)] Redis bytes, the keys as bloom_pack_keys gives them, rows [nq][cap],
    slots [nq] → [nq][cap] uint8.  No context, no device."""
    bs, sd, ko, kb, r, cnt, sl = _bloom_host_args("bloom_exists_host", m, k, seeds, bitsets, key_offsets, key_bytes, rows, count, slots)
    out = np.empty(r.shape, dtype=np.uint8)
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_bloom_exists_host(int(m), int(k), v(sd), bs.shape[0], _ptr(bs), ko.shape[0] - 1, _ptr(ko), _ptr(kb), r.shape[0],
                                                r.shape[1], _ptr(r), v(cnt), _ptr(sl), _ptr(out)))
    return out


def bloom_add_host(m: int, k: int, seeds, bitsets: np.ndarray, key_offsets, key_bytes, rows, slots, count=None) -> None:
    """pg_bloom_add_host: sets the bits in `bitsets` (a C-contiguous uint8 array [n_slots][ceil(m / 8)]) in place."""
    if not (isinstance(bitsets, np.ndarray) and bitsets.dtype == np.uint8 and bitsets.flags.c_contiguous and bitsets.flags.writeable):
        raise TypeError("bloom_add_host: bitsets is a writable C-contiguous uint8 array")
    bs, sd, ko, kb, r, cnt, sl = _bloom_host_args("bloom_add_host", m, k, seeds, bitsets, key_offsets, key_bytes, rows, count, slots)
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_bloom_add_host(int(m), int(k), v(sd), bs.shape[0], _ptr(bs), ko.shape[0] - 1, _ptr(ko), _ptr(kb), r.shape[0],
                                             r.shape[1], _ptr(r), v(cnt), _ptr(sl)))


def bloom_filter_host(m: int, k: int, seeds, bitsets, key_offsets, key_bytes, slots, rows, score, source=None, count=None, planes_f64=None,
                      source_mask=None, planes_f32=None):
    """pg_bloom_filter_host: the filter on host arrays by the library's host statement; the lists and the result as
    Context.bloom_filter."""
    nq, cap, ins, outs, n64, n32 = _cand_arrays("bloom_filter_host", lambda cap: cap, rows, score, source, count, planes_f64, source_mask,
                                                planes_f32)
    bs, sd, ko, kb, r, cnt, sl = _bloom_host_args("bloom_filter_host", m, k, seeds, bitsets, key_offsets, key_bytes, ins[0], ins[3], slots)
    v = lambda a: None if a is None else _ptr(a)                                     # noqa: E731
    _lib.check(_lib.load().pg_bloom_filter_host(int(m), int(k), v(sd), bs.shape[0], _ptr(bs), ko.shape[0] - 1, _ptr(ko), _ptr(kb), nq, cap,
                                                v(ins[0]), v(ins[1]), v(ins[2]), v(ins[3]), v(ins[4]), n64, v(ins[5]), v(ins[6]), n32, _ptr(sl),
                                                *[v(a) for a in outs]))
    return tuple(outs)


def bloom_slot_write_host(m: int, bitsets: np.ndarray, slot: int, data) -> None:
    """pg_bloom_slot_write_host: pg_bloom_slot_write on a host bitset array [n_slots][ceil(m / 8)], in place."""
    if not (isinstance(bitsets, np.ndarray) and bitsets.dtype == np.uint8 and bitsets.flags.c_contiguous and bitsets.ndim == 2):
        raise TypeError("bloom_slot_write_host: bitsets is a C-contiguous uint8 array [n_slots][ceil(m / 8)]")
    d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    _lib.check(_lib.load().pg_bloom_slot_write_host(int(m), bitsets.shape[0], _ptr(bitsets), int(slot), _ptr(d) if d.size else None, d.size))


class BloomKeys:
    """pg_bloom_keys: the bytes each item-table row is hashed by (the item id string), uploaded once.  keys: a sequence of bytes
    objects, or ids=[...] for the decimal text of integer ids."""

    def __init__(self, ctx: "Context", keys=None, ids=None):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        if ids is not None:
            a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            _lib.check(self.L.pg_bloom_keys_create_decimal(ctx.h, a.shape[0], _ptr(a) if a.size else None, C.byref(h)))
            self.rows = a.shape[0]
        else:
            off, data = bloom_pack_keys(keys)
            _lib.check(self.L.pg_bloom_keys_create(ctx.h, off.shape[0] - 1, _ptr(off), _ptr(data) if data.size else None, C.byref(h)))
            self.rows = off.shape[0] - 1
        self.h = h

    def free(self):
        if self.h:
            _lib.check(self.L.pg_bloom_keys_free(self.ctx.h, self.h))
            self.h = None


class Bloom:
    """pg_bloom: n_slots Bloom bitsets of m bits in HBM, k murmur3 hashes per key (seeds None: the first k primes)."""

    def __init__(self, ctx: "Context", m: int, k: int, n_slots: int, seeds=None):
        self.ctx, self.L = ctx, ctx.L
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
        if sd is not None and sd.shape != (k,):
            raise ValueError("Bloom: one seed per hash")
        h = C.c_void_p()
        _lib.check(self.L.pg_bloom_create(ctx.h, int(m), int(k), _ptr(sd) if sd is not None else None, int(n_slots), C.byref(h)))
        self.h = h
        self.m, self.k, self.n_slots = int(m), int(k), int(n_slots)
        self.nbytes = (self.m + 7) // 8

    def free(self):
        if self.h:
            _lib.check(self.L.pg_bloom_free(self.ctx.h, self.h))
            self.h = None

    def info(self) -> dict:
        m, k, n, b = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        _lib.check(self.L.pg_bloom_info(self.h, C.byref(m), C.byref(k), C.byref(n), C.byref(b)))
        return {"m": m.value, "k": k.value, "n_slots": n.value, "slot_bytes": b.value}

    def slot_write(self, slot: int, data) -> None:
        """pg_bloom_slot_write: up to ceil(m / 8) Redis-order bytes (a user's Redis value as it is); the rest of the slot is zeroed"""
        d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        _lib.check(self.L.pg_bloom_slot_write(self.ctx.h, self.h, int(slot), _ptr(d) if d.size else None, d.size))

    def slot_read(self, slot: int, n: Optional[int] = None) -> np.ndarray:
        """pg_bloom_slot_read → the slot's first n (default: all ceil(m / 8)) Redis-order bytes"""
        out = np.empty(self.nbytes if n is None else int(n), dtype=np.uint8)
        _lib.check(self.L.pg_bloom_slot_read(self.ctx.h, self.h, int(slot), _ptr(out) if out.size else None, out.size))
        return out

    def slot_clear(self, slot: int) -> None:
        _lib.check(self.L.pg_bloom_slot_clear(self.ctx.h, self.h, int(slot)))


class ColdStart:
    """ColdStartRecall (pg_cold_*): the rows a clause admits as a recall answer — a keyed uniform sample per request (order_by
    None, "" or "random()") or the head of the pool by one column ("create_time DESC").  `where` is borrowed (None: every row of
    the table) and must outlive this object; creating needs no GPU."""

    def __init__(self, where: Optional[Where] = None, order_by: Optional[str] = None):
        self.L = _lib.load()
        self.where = where
        h = C.c_void_p()
        _lib.check(self.L.pg_cold_create(where.h if where is not None else None,
                                         order_by.encode("utf-8") if order_by is not None else None, C.byref(h)))
        self.h = h

    def free(self):
        if self.h:
            self.L.pg_cold_free(self.h)
            self.h = None

    @staticmethod
    def _seeds(seed, nq: int):
        if seed is None:
            return None
        s = np.ascontiguousarray(seed, dtype=np.uint64)
        if s.shape != (nq,):
            raise ValueError("ColdStart: one seed per request")
        return s

    def recall_host(self, rows: int, nq: int, k: int, bits: Optional[np.ndarray] = None, order_col: Optional[np.ndarray] = None,
                    seed=None, row_offset: int = 0):
        """The host statement (pg_cold_recall_host): bits = the clause's bitmap over `rows` rows (Where.eval_host; None: every
        row), order_col = the ordered column's values (int32 / int64 / float32 / float64) → (rows [nq][k] u64, scores [nq][k]
        f32, counts [nq] u32)."""
        b = None if bits is None else np.ascontiguousarray(bits, dtype=np.uint32)
        if b is not None and b.shape[0] < (rows + 31) // 32:
            raise ValueError("ColdStart.recall_host: the bitmap is shorter than the rows")
        oc, dt = None, 0
        if order_col is not None:
            oc = np.ascontiguousarray(order_col)
            dts = [d for d, t in _F_NP.items() if oc.dtype == t]
            if not dts or oc.shape != (rows,):
                raise TypeError("ColdStart.recall_host: the order column is one int32 / int64 / float32 / float64 value per row")
            dt = dts[0]
        s = self._seeds(seed, nq)
        out_r = np.empty((nq, k), dtype=np.uint64)
        out_s = np.empty((nq, k), dtype=np.float32)
        cnt = np.empty(nq, dtype=np.uint32)
        _lib.check(self.L.pg_cold_recall_host(self.h, _ptr(b) if b is not None else None, rows, row_offset,
                                              _ptr(oc) if oc is not None else None, dt, _ptr(s) if s is not None else None, nq, k,
                                              _ptr(out_r), _ptr(out_s), _ptr(cnt)))
        return out_r, out_s, cnt

    def recall_dev(self, ctx: "Context", table: "Table", feats: Optional["Features"], d_seed: int, nq: int, k: int, d_out_rows: int,
                   d_out_scores: int, d_out_count: int = 0) -> None:
        """pg_cold_recall_dev: device addresses (d_seed 0 = seed 0 for every request), enqueued on the context's stream."""
        _lib.check(self.L.pg_cold_recall_dev(ctx.h, self.h, table.h, feats.h if feats is not None else None, C.c_void_p(d_seed or None),
                                             nq, k, C.c_void_p(d_out_rows or None), C.c_void_p(d_out_scores or None),
                                             C.c_void_p(d_out_count or None)))

    def recall(self, ctx: "Context", table: "Table", feats: Optional["Features"], nq: int, k: int, seed=None):
        """pg_cold_recall on host arrays → (rows [nq][k] u64, scores [nq][k] f32, counts [nq] u32)"""
        s = self._seeds(seed, nq)
        out_r = np.empty((max(nq, 1), max(k, 1)), dtype=np.uint64)
        out_s = np.empty((max(nq, 1), max(k, 1)), dtype=np.float32)
        cnt = np.empty(max(nq, 1), dtype=np.uint32)
        _lib.check(self.L.pg_cold_recall(ctx.h, self.h, table.h, feats.h if feats is not None else None,
                                         _ptr(s) if s is not None else None, nq, k, _ptr(out_r), _ptr(out_s), _ptr(cnt)))
        return out_r, out_s, cnt

    def stats(self) -> dict:
        st = _lib.PgColdStats()
        _lib.check(self.L.pg_cold_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}


class Expr:
    """Compiled RankConfig.RankScore expression (utils/ast replacement)."""

    def __init__(self, source: str, ast_type: str = "", govaluate: bool = False):
        """ast_type "antlr": the subset of the reference's second evaluator (pg_expr_compile_typed); govaluate: the arithmetic
        subset of govaluate that BoostScoreSort expressions use (pg_expr_compile_govaluate)."""
        self.L = _lib.load()
        h = C.c_void_p()
        if govaluate:
            _lib.check(self.L.pg_expr_compile_govaluate(source.encode("utf-8"), C.byref(h)))
        elif ast_type:
            _lib.check(self.L.pg_expr_compile_typed(source.encode("utf-8"), ast_type.encode("utf-8"), C.byref(h)))
        else:
            _lib.check(self.L.pg_expr_compile(source.encode("utf-8"), C.byref(h)))
        self.h = h
        n = self.L.pg_expr_num_vars(h)
        self.var_names = [self.L.pg_expr_var_name(h, i).decode("utf-8") for i in range(n)]

    def free(self):
        if self.h:
            self.L.pg_expr_free(self.h)
            self.h = None

    def set_score_rewrites(self, rewrites: dict):
        """RankConfig.ScoreRewrite {source: expression} of the scene this RankScore belongs to (pg_expr_set_score_rewrites).
        An expression that does not compile is passed as NULL — the reference scores such a source 0."""
        names = list(rewrites.keys())
        exprs = []
        for nm in names:
            try:
                exprs.append(Expr(rewrites[nm]))
            except _lib.PgError:
                exprs.append(None)
        arr_n = (C.c_char_p * max(len(names), 1))(*[nm.encode("utf-8") for nm in names])
        arr_e = (C.c_void_p * max(len(names), 1))(*[(x.h if x is not None else None) for x in exprs])
        try:
            _lib.check(self.L.pg_expr_set_score_rewrites(self.h, len(names), arr_n, arr_e))
        finally:
            for x in exprs:
                if x is not None:
                    x.free()

    def eval_host(self, vars_: np.ndarray) -> np.ndarray:
        """pg_expr_eval_host: the program on host arrays (no context, no device); vars_ as eval."""
        v = np.ascontiguousarray(vars_, dtype=np.float64).reshape(len(self.var_names), -1) \
            if len(self.var_names) else np.zeros((0, int(np.shape(vars_)[-1])), dtype=np.float64)
        n = v.shape[1]
        out = np.empty(n, dtype=np.float64)
        _lib.check(self.L.pg_expr_eval_host(self.h, _ptr(v) if v.size else None, n, _ptr(out)))
        return out

    def eval(self, ctx: Context, vars_: np.ndarray) -> np.ndarray:
        """vars_: [n_vars][n_items] fp64 in var_names order → fused scores [n_items] fp64."""
        v = np.ascontiguousarray(vars_, dtype=np.float64).reshape(len(self.var_names), -1) \
            if len(self.var_names) else np.zeros((0, int(np.shape(vars_)[-1])), dtype=np.float64)
        n = v.shape[1]
        out = np.empty(n, dtype=np.float64)
        _lib.check(self.L.pg_expr_eval(ctx.h, self.h, _ptr(v) if v.size else None, n, _ptr(out)))
        return out


def recommend_dnn3(ctx: Context, table: Table, model: "RankModel", expr: "Expr", rank_var: str, queries: np.ndarray,
                   k: int):
    """pg_recommend_dnn3_dev on host arrays (tests, tools): queries [R][dim] →
    rows [R][k] u64, recall scores [R][k] f32, model scores [R][k] f32, fused [R][k] f64, order [R][k] u32, counts [R]."""
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, table.dim)
    R = q.shape[0]
    n = R * k
    d_q = ctx.to_device(q)
    bufs = [ctx.malloc(n * 8), ctx.malloc(n * 4), ctx.malloc(n * 4), ctx.malloc(n * 8), ctx.malloc(n * 4),
            ctx.malloc(max(R * 4, 16))]
    try:
        _lib.check(ctx.L.pg_recommend_dnn3_dev(ctx.h, table.h, model.h, expr.h, rank_var.encode(), d_q, R, k, *bufs))
        outs = [np.zeros((R, k), np.uint64), np.zeros((R, k), np.float32), np.zeros((R, k), np.float32),
                np.zeros((R, k), np.float64), np.zeros((R, k), np.uint32), np.zeros(R, np.uint32)]
        for a, p_ in zip(outs, bufs):
            ctx.d2h(a, p_)
    finally:
        for p_ in [d_q] + bufs:
            ctx.free(p_)
    return tuple(outs)


def recommend_candidates_dnn3(ctx: Context, table: Table, model: "RankModel", expr: "Expr", rank_var: str, user_vecs: np.ndarray,
                              rows: np.ndarray, score: np.ndarray, count=None):
    """pg_recommend_candidates_dnn3_dev on host arrays: the stages behind the recall for candidate lists the caller made
    (Context.fanin_merge's rows / score / count): user_vecs [R][dim], rows [R][cap] u64, score [R][cap] f64, count [R] or None →
    model scores [R][cap] f32, fused [R][cap] f64, order [R][cap] u32."""
    u = np.ascontiguousarray(user_vecs, dtype=np.float32).reshape(-1, table.dim)
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    sc = np.ascontiguousarray(score, dtype=np.float64)
    R, cap = r.shape
    if sc.shape != r.shape or u.shape[0] != R:
        raise ValueError("recommend_candidates_dnn3: rows and score are [R][cap], user_vecs [R][dim]")
    n = R * cap
    ins = [ctx.to_device(u), ctx.to_device(r), ctx.to_device(sc),
           ctx.to_device(np.ascontiguousarray(count, dtype=np.uint32)) if count is not None else 0]
    bufs = [ctx.malloc(max(n * 4, 16)), ctx.malloc(max(n * 8, 16)), ctx.malloc(max(n * 4, 16))]
    try:
        _lib.check(ctx.L.pg_recommend_candidates_dnn3_dev(ctx.h, table.h, model.h, expr.h, rank_var.encode(), ins[0], R, cap, ins[1], ins[2],
                                                          ins[3] or None, *bufs))
        outs = [np.zeros((R, cap), np.float32), np.zeros((R, cap), np.float64), np.zeros((R, cap), np.uint32)]
        for a, p_ in zip(outs, bufs):
            ctx.d2h(a, p_)
    finally:
        for p_ in ins + bufs:
            if p_:
                ctx.free(p_)
    return tuple(outs)


def recommend_cascade_dnn3(ctx: Context, table: Table, coarse: "RankModel", e_coarse: "Expr", coarse_var: str, fine: "RankModel",
                           e_fine: "Expr", fine_var: str, user_vecs: np.ndarray, rows: np.ndarray, score: np.ndarray, n_keep: int,
                           source=None, count=None):
    """pg_recommend_cascade_dnn3_dev on host arrays: coarse rank → fusion → sort → keep n_keep → fine rank → fusion → sort over
    candidate lists the caller made (inputs as recommend_candidates_dnn3, plus source [R][cap] u8 or None) → rows [R][n_keep] u64,
    coarse fused [R][n_keep] f64, coarse model scores f32, source u8 or None, fine model scores f32, fine fused f64, order u32,
    count [R] u32."""
    u = np.ascontiguousarray(user_vecs, dtype=np.float32).reshape(-1, table.dim)
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    sc = np.ascontiguousarray(score, dtype=np.float64)
    R, cap = r.shape
    if sc.shape != r.shape or u.shape[0] != R:
        raise ValueError("recommend_cascade_dnn3: rows and score are [R][cap], user_vecs [R][dim]")
    nk = R * max(int(n_keep), 0)
    ins = [ctx.to_device(u), ctx.to_device(r), ctx.to_device(sc),
           ctx.to_device(np.ascontiguousarray(source, dtype=np.uint8)) if source is not None else 0,
           ctx.to_device(np.ascontiguousarray(count, dtype=np.uint32)) if count is not None else 0]
    # rows, coarse fused, source, model scores [2], fused, order, count
    sizes = [nk * 8, nk * 8, nk if source is not None else 0, 2 * nk * 4, nk * 8, nk * 4, R * 4]
    bufs = [ctx.malloc(max(b, 16)) if b or i != 2 else 0 for i, b in enumerate(sizes)]
    try:
        _lib.check(ctx.L.pg_recommend_cascade_dnn3_dev(ctx.h, table.h, coarse.h, e_coarse.h, coarse_var.encode(), fine.h, e_fine.h,
                                                       fine_var.encode(), ins[0], R, cap, ins[1], ins[2], ins[3] or None, ins[4] or None,
                                                       int(n_keep), bufs[0], bufs[1], bufs[2] or None, *bufs[3:]))
        outs = [np.zeros((R, n_keep), np.uint64), np.zeros((R, n_keep), np.float64),
                np.zeros((R, n_keep), np.uint8) if source is not None else None, np.zeros((2, R, n_keep), np.float32),
                np.zeros((R, n_keep), np.float64), np.zeros((R, n_keep), np.uint32), np.zeros(R, np.uint32)]
        for a, p_ in zip(outs, bufs):
            if a is not None:
                ctx.d2h(a, p_)
    finally:
        for p_ in ins + bufs:
            if p_:
                ctx.free(p_)
    rows_o, c_fused, src_o, ms, fused, order, cnt = outs
    return rows_o, c_fused, ms[1], src_o, ms[0], fused, order, cnt

class Coalescer:
    """Cross-request batching (pg_coalescer_*): every method serves ONE request and may be called from any number
    of threads at once (ctypes releases the GIL for the duration of the call); the library forms the batches.

    Two ways to build one: the single-DNN form (model / expr / rank_var: pg_coalescer_create), or a scene
    (`algos` = [(name, RankModel) or (name, RankModel, Features, item field column names)], expr, `dpp` =
    {"candidates": C, "alpha": a, "window": w, "normalize_emb": True, "norm_relevance_score": 0},
    query_model, trigger_table: pg_coalescer_create_scene)."""

    def __init__(self, ctx: Context, table: Table, k: int, model: Optional["RankModel"] = None,
                 expr: Optional["Expr"] = None, rank_var: str = "", max_batch: int = 0, max_wait_us: int = 0,
                 depth: int = 0, max_top_n: int = 0, max_rank_items: int = 0, timeout_us: int = 0,
                 algos=None, dpp: Optional[dict] = None, query_model: Optional["RankModel"] = None,
                 trigger_table: Optional[Table] = None, max_rerank_items: int = 0, max_hook_dim: int = 0):
        self.ctx, self.table, self.k = ctx, table, k
        self.max_top_n = max_top_n or k
        cfg = _lib.PgCoalescerConfig(k, max_batch, max_wait_us, depth, max_top_n, max_rank_items, timeout_us)
        h = C.c_void_p()
        scene = algos is not None or dpp is not None or query_model is not None or trigger_table is not None \
            or max_rerank_items or max_hook_dim
        self.n_algos = 1 if model else 0
        self.n_planes = getattr(model, "n_out", 1) if model else 0
        self.algo_outputs = [self.n_planes] if model else []
        self.dnn_heads = self.n_planes or 1
        if not scene:
            _lib.check(ctx.L.pg_coalescer_create(ctx.h, table.h, model.h if model else None, expr.h if expr else None,
                                                 rank_var.encode() if rank_var else None, C.byref(cfg), C.byref(h)))
        else:
            if algos is None:
                algos = [(rank_var, model)] if model else []
            arr = (_lib.PgRankAlgo * max(len(algos), 1))()
            self._keep = []
            for i, a in enumerate(algos):
                name, m = a[0], a[1]
                nm = name.encode()
                self._keep.append(nm)
                arr[i].model = m.h
                arr[i].name = nm
                if len(a) == 3 and isinstance(a[2], (list, tuple)):     # (name, multi-output model, output names)
                    onames = (C.c_char_p * len(a[2]))(*[str(x).encode() for x in a[2]])
                    self._keep.append(onames)
                    arr[i].output_names = onames
                elif len(a) == 3:                     # (name, model, ItemRows)
                    arr[i].item_rows = a[2].h
                elif len(a) > 3:                      # (name, model, Features, item field column names)
                    feats, cols = a[2], a[3]
                    idx = feats._cols(cols)
                    carr = (C.c_int32 * len(idx))(*[int(x) for x in idx])
                    self._keep.append(carr)
                    arr[i].features = feats.h
                    arr[i].item_field_cols = carr
            sc = _lib.PgSceneConfig()
            sc.base = cfg
            sc.algos = arr
            sc.n_algos = len(algos)
            sc.rank_score = expr.h if expr else None
            if dpp is not None:
                sc.rerank = 1
                sc.rerank_candidates = int(dpp["candidates"])
                sc.dpp = _lib.PgDppOptions(float(dpp.get("alpha", 1.0)), 0, int(dpp.get("window", 10)),
                                           int(dpp.get("normalize_emb", True)), 1,
                                           int(dpp.get("norm_relevance_score", 0)), 1, 0)
            sc.query_model = query_model.h if query_model else None
            sc.trigger_table = trigger_table.h if trigger_table else None
            sc.max_rerank_items = max_rerank_items
            sc.max_hook_dim = max_hook_dim
            self.n_algos = len(algos)
            self.n_planes = sum(getattr(a[1], "n_out", 1) for a in algos)
            self.algo_outputs = [getattr(a[1], "n_out", 1) for a in algos]
            self.dnn_heads = next((a[1].n_out for a in algos if a[1].kind in (MODEL_DNN3, MODEL_DNN3_MULTI)), 1)
            _lib.check(ctx.L.pg_coalescer_create_scene(ctx.h, table.h, C.byref(sc), C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_coalescer_destroy(self.h))
            self.h = None

    def _recall_out(self):
        return np.empty(self.k, dtype=np.uint64), np.empty(self.k, dtype=np.float32), C.c_uint32()

    def recall(self, query: np.ndarray):
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.table.dim)
        rows, scores, cnt = self._recall_out()
        _lib.check(self.ctx.L.pg_coalescer_recall(self.h, _ptr(q), _ptr(rows), _ptr(scores), C.byref(cnt)))
        return rows, scores, cnt.value

    def recall_l2(self, query: np.ndarray):
        """HologresVectorRecallV2: one request; (rows, squared Euclidean distances ascending, count)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.table.dim)
        rows, dist, cnt = self._recall_out()
        _lib.check(self.ctx.L.pg_coalescer_recall_l2(self.h, _ptr(q), _ptr(rows), _ptr(dist), C.byref(cnt)))
        return rows, dist, cnt.value

    def recall_exclude(self, query: np.ndarray, ids):
        """one request without the global row ids it has seen (pg_coalescer_recall_exclude; the context option
        "coalescer_max_exclude" must be set when the coalescer is created)"""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.table.dim)
        x = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        rows, scores, cnt = self._recall_out()
        _lib.check(self.ctx.L.pg_coalescer_recall_exclude(self.h, _ptr(q), _ptr(x), x.shape[0], _ptr(rows), _ptr(scores), C.byref(cnt)))
        return rows, scores, cnt.value

    def i2i_recall(self, trigger_row: int):
        rows, scores, cnt = self._recall_out()
        _lib.check(self.ctx.L.pg_coalescer_i2i_recall(self.h, int(trigger_row), _ptr(rows), _ptr(scores), C.byref(cnt)))
        return rows, scores, cnt.value

    def online_recall(self, user_vec: np.ndarray):
        u = np.ascontiguousarray(user_vec, dtype=np.float32).reshape(-1)
        rows, scores, cnt = self._recall_out()
        _lib.check(self.ctx.L.pg_coalescer_online_recall(self.h, _ptr(u), _ptr(rows), _ptr(scores), C.byref(cnt)))
        return rows, scores, cnt.value

    def rank_dnn3(self, user_vec: np.ndarray, cand_rows: np.ndarray) -> np.ndarray:
        u = np.ascontiguousarray(user_vec, dtype=np.float32).reshape(-1)
        c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        heads = getattr(self, "dnn_heads", 1)
        out = np.empty((heads, c.shape[0]), dtype=np.float32)
        _lib.check(self.ctx.L.pg_coalescer_rank_dnn3(self.h, _ptr(u), _ptr(c), c.shape[0], _ptr(out)))
        return out[0] if heads == 1 else out

    def rank(self, algo: int, user_vec: np.ndarray, cand_rows: np.ndarray, user_field_ids=None) -> np.ndarray:
        u = np.ascontiguousarray(user_vec, dtype=np.float32).reshape(-1)
        c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        uf = None if user_field_ids is None else np.ascontiguousarray(user_field_ids, dtype=np.int32)
        heads = self.algo_outputs[algo]
        out = np.empty((heads, c.shape[0]), dtype=np.float32)
        _lib.check(self.ctx.L.pg_coalescer_rank(self.h, algo, _ptr(u), _ptr(uf) if uf is not None else None, _ptr(c),
                                                c.shape[0], _ptr(out)))
        return out[0] if heads == 1 else out

    def rank_fm2t(self, user_vec: np.ndarray, user_field_ids, cand_rows: np.ndarray) -> np.ndarray:
        u = np.ascontiguousarray(user_vec, dtype=np.float32).reshape(-1)
        uf = np.ascontiguousarray(user_field_ids, dtype=np.int32)
        c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        out = np.empty(c.shape[0], dtype=np.float32)
        _lib.check(self.ctx.L.pg_coalescer_rank_fm2t(self.h, _ptr(u), _ptr(uf), _ptr(c), c.shape[0], _ptr(out)))
        return out

    def recommend(self, user_vec: np.ndarray, top_n: int, user_field_ids=None):
        """→ (rows, recall scores, model scores, fused scores) of the page (the first top_n entries of the sorted list,
        or DPPSort's picks when the scene has the stage), count.  With several rank algorithms (or user_field_ids)
        the model scores are [n_algos][top_n]."""
        u = np.ascontiguousarray(user_vec, dtype=np.float32).reshape(self.table.dim)
        rows = np.empty(top_n, dtype=np.uint64)
        rec = np.empty(top_n, dtype=np.float32)
        fus = np.empty(top_n, dtype=np.float64)
        cnt = C.c_uint32()
        if user_field_ids is None and self.n_planes <= 1:
            rnk = np.empty(top_n, dtype=np.float32)
            _lib.check(self.ctx.L.pg_coalescer_recommend(self.h, _ptr(u), top_n, _ptr(rows), _ptr(rec), _ptr(rnk),
                                                         _ptr(fus), C.byref(cnt)))
        else:
            rnk = np.empty((self.n_planes, top_n), dtype=np.float32)
            uf = None if user_field_ids is None else np.ascontiguousarray(user_field_ids, dtype=np.int32)
            _lib.check(self.ctx.L.pg_coalescer_recommend_ex(self.h, _ptr(u), _ptr(uf) if uf is not None else None, top_n,
                                                            _ptr(rows), _ptr(rec), _ptr(rnk), _ptr(fus), C.byref(cnt)))
        return rows, rec, rnk, fus, cnt.value

    def dpp(self, cand_rows, rel, alpha: float, topn: int, window: int, normalize_emb: bool = True,
            ensure_pos_similarity: bool = True, norm_relevance_score: int = 0, hook_emb: Optional[np.ndarray] = None,
            has_table: bool = True):
        """pg_coalescer_dpp: one request's DPPSort; → (picked indices, relevance scores as used)."""
        r = np.ascontiguousarray(rel, dtype=np.float64)
        n = r.shape[0]
        c = np.ascontiguousarray(cand_rows, dtype=np.uint32) if has_table else None
        hk = None if hook_emb is None else np.ascontiguousarray(hook_emb, dtype=np.float64).reshape(n, -1)
        opt = _lib.PgDppOptions(alpha, topn, window, int(normalize_emb), int(ensure_pos_similarity),
                                int(norm_relevance_score), int(has_table), 0 if hk is None else hk.shape[1])
        out = np.zeros(max(topn, 1), dtype=np.uint32)
        used = np.zeros(max(n, 1), dtype=np.float64)
        cnt = C.c_uint32()
        _lib.check(self.ctx.L.pg_coalescer_dpp(self.h, _ptr(c) if c is not None else None, _ptr(r), n, C.byref(opt),
                                               _ptr(hk) if hk is not None else None, _ptr(out), C.byref(cnt), _ptr(used)))
        return out[:cnt.value], used[:n]

    def ssd(self, cand_rows, rel, gamma: float, topn: int, window: int, normalize_emb: bool = True,
            ensure_pos_similarity: bool = True, norm_quality_score: int = 0, use_ssd_star: bool = False):
        """pg_coalescer_ssd: one request's SSDSort; → (picked indices, quality scores)."""
        c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
        r = np.ascontiguousarray(rel, dtype=np.float64)
        out = np.zeros(max(c.shape[0], 1), dtype=np.uint32)
        qual = np.zeros(max(c.shape[0], 1), dtype=np.float64)
        cnt = C.c_uint32()
        _lib.check(self.ctx.L.pg_coalescer_ssd(self.h, _ptr(c), _ptr(r), c.shape[0], gamma, topn, window, int(normalize_emb),
                                               int(ensure_pos_similarity), int(norm_quality_score), int(use_ssd_star),
                                               _ptr(out), C.byref(cnt), _ptr(qual)))
        return out[:cnt.value], qual[:c.shape[0]]

    def stats(self) -> _lib.PgCoalescerStats:
        s = _lib.PgCoalescerStats()
        _lib.check(self.ctx.L.pg_coalescer_stats(self.h, C.byref(s)))
        return s


class GroupCoalescer(Coalescer):
    """pg_coalescer_create_group: single-request recommend calls batched into steps of a shard group."""

    def __init__(self, group: "ShardGroup", expr: "Expr", rank_var: str, k: int, max_top_n: int = 0, dpp_candidates: int = 0,
                 dpp_alpha: float = 1.0, dpp_window: int = 10, dpp_normalize_emb: bool = True, max_batch: int = 0,
                 max_wait_us: int = 0, depth: int = 0, timeout_us: int = 0):
        self.L = group.L
        self.group, self.k, self.n_algos = group, k, 1
        self.n_planes, self.algo_outputs, self.dnn_heads = 1, [1], 1
        self.max_top_n = max_top_n or k
        plan = _lib.PgGroupPlan(k, dpp_candidates, dpp_alpha, dpp_window, int(dpp_normalize_emb))
        cfg = _lib.PgCoalescerConfig(k, max_batch, max_wait_us, depth, max_top_n, 0, timeout_us)
        h = C.c_void_p()
        _lib.check(self.L.pg_coalescer_create_group(group.h, expr.h, rank_var.encode(), C.byref(plan), C.byref(cfg), C.byref(h)))
        self.h = h

        class _T:          # (what Coalescer.recommend reads off its table / context)
            dim = group.dim
        self.table = _T()

        class _Cx:
            L = group.L
        self.ctx = _Cx()


class Router:
    """pg_router_*: per-request calls spread over replica coalescers (least outstanding requests first)."""

    def __init__(self, replicas: Sequence["Coalescer"]):
        self.L = _lib.load()
        self.replicas = list(replicas)
        arr = (C.c_void_p * len(replicas))(*[r.h for r in replicas])
        h = C.c_void_p()
        _lib.check(self.L.pg_router_create(arr, len(replicas), C.byref(h)))
        self.h = h
        self.dim = replicas[0].table.dim
        self.k = replicas[0].k

    def destroy(self):
        if self.h:
            self.L.pg_router_destroy(self.h)
            self.h = None

    def recommend(self, user_vec: np.ndarray, top_n: int):
        u = np.ascontiguousarray(user_vec, dtype=np.float32).reshape(self.dim)
        rows = np.empty(top_n, dtype=np.uint64)
        rec = np.empty(top_n, dtype=np.float32)
        rnk = np.empty(top_n, dtype=np.float32)
        fus = np.empty(top_n, dtype=np.float64)
        cnt = C.c_uint32()
        _lib.check(self.L.pg_router_recommend(self.h, _ptr(u), top_n, _ptr(rows), _ptr(rec), _ptr(rnk), _ptr(fus), C.byref(cnt)))
        return rows, rec, rnk, fus, cnt.value

    def recall(self, query: np.ndarray):
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.dim)
        rows = np.empty(self.k, dtype=np.uint64)
        scores = np.empty(self.k, dtype=np.float32)
        cnt = C.c_uint32()
        _lib.check(self.L.pg_router_recall(self.h, _ptr(q), _ptr(rows), _ptr(scores), C.byref(cnt)))
        return rows, scores, cnt.value

    def served(self) -> np.ndarray:
        out = (C.c_uint64 * len(self.replicas))()
        _lib.check(self.L.pg_router_stats(self.h, out))
        out = np.array(list(out), dtype=np.uint64)
        return out


class ShardGroup:
    """pg_group_*: the item table in row-range shards over several GPUs of this process (or logical shards of one)."""

    def __init__(self, devices: Sequence[int]):
        self.L = _lib.load()
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _lib.check(self.L.pg_group_create(arr, len(devices), C.byref(h)))
        self.h, self.n = h, len(devices)
        self.dim = 0

    def destroy(self):
        if self.h:
            _lib.check(self.L.pg_group_destroy(self.h))
            self.h = None

    def table_create(self, total_rows: int, dim: int):
        _lib.check(self.L.pg_group_table_create(self.h, total_rows, dim))
        self.dim = dim

    def table_fill_synthetic(self, seed: int, normalize: bool = True):
        _lib.check(self.L.pg_group_table_fill_synthetic(self.h, seed, int(normalize)))

    def table_upload(self, rows: np.ndarray, row0: int = 0):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        _lib.check(self.L.pg_group_table_upload(self.h, row0, rows.shape[0], _ptr(rows)))

    def model_load(self, kind: int, prec: int, blob: bytes):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        _lib.check(self.L.pg_group_model_load(self.h, kind, prec, buf, len(blob)))

    def recommend(self, expr: "Expr", rank_var: str, user_vecs: np.ndarray, k: int, top_n: int,
                  dpp_candidates: int = 0, dpp_alpha: float = 1.0, dpp_window: int = 10,
                  dpp_normalize_emb: bool = True):
        u = np.ascontiguousarray(user_vecs, dtype=np.float32).reshape(-1, self.dim)
        nq = u.shape[0]
        plan = _lib.PgGroupPlan(k, dpp_candidates, dpp_alpha, dpp_window, int(dpp_normalize_emb))
        rows = np.empty((nq, top_n), dtype=np.uint64)
        rec = np.empty((nq, top_n), dtype=np.float32)
        rnk = np.empty((nq, top_n), dtype=np.float32)
        fus = np.empty((nq, top_n), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.L.pg_group_recommend(self.h, expr.h, rank_var.encode(), C.byref(plan), _ptr(u), nq, top_n,
                                             _ptr(rows), _ptr(rec), _ptr(rnk), _ptr(fus), _ptr(cnt)))
        return rows, rec, rnk, fus, cnt


    def recommend_begin(self, expr: "Expr", rank_var: str, user_vecs: np.ndarray, k: int, top_n: int,
                        dpp_candidates: int = 0, dpp_alpha: float = 1.0, dpp_window: int = 10,
                        dpp_normalize_emb: bool = True):
        """pg_group_recommend_begin: enqueue a step, return its ticket (up to two may be outstanding)."""
        u = np.ascontiguousarray(user_vecs, dtype=np.float32).reshape(-1, self.dim)
        plan = _lib.PgGroupPlan(k, dpp_candidates, dpp_alpha, dpp_window, int(dpp_normalize_emb))
        tk = C.c_void_p()
        _lib.check(self.L.pg_group_recommend_begin(self.h, expr.h, rank_var.encode(), C.byref(plan), _ptr(u), u.shape[0], top_n,
                                                   C.byref(tk)))
        return (tk, u.shape[0], top_n)

    def exchange_stats(self) -> dict:
        """the first exchange: steps served, steps repeated with the whole lists, bytes per shard and peer and entries per request in the last step"""
        a = (C.c_uint64 * 4)()
        _lib.check(self.L.pg_group_exchange_stats(self.h, a))
        return {"steps": int(a[0]), "round2_steps": int(a[1]), "exchange1_bytes_per_shard": int(a[2]), "entries_per_request_and_shard": int(a[3])}

    def recommend_end(self, ticket):
        tk, nq, top_n = ticket
        rows = np.empty((nq, top_n), dtype=np.uint64)
        rec = np.empty((nq, top_n), dtype=np.float32)
        rnk = np.empty((nq, top_n), dtype=np.float32)
        fus = np.empty((nq, top_n), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.uint32)
        _lib.check(self.L.pg_group_recommend_end(self.h, tk, _ptr(rows), _ptr(rec), _ptr(rnk), _ptr(fus), _ptr(cnt)))
        return rows, rec, rnk, fus, cnt


def dpp(ctx: Context, table: Table, cand_rows, rel, alpha: float, topn: int, window: int,
        normalize_emb: bool = True) -> np.ndarray:
    c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
    r = np.ascontiguousarray(rel, dtype=np.float64)
    out = np.zeros(max(topn, 1), dtype=np.uint32)
    cnt = C.c_uint32()
    _lib.check(ctx.L.pg_dpp(ctx.h, table.h, _ptr(c), _ptr(r), c.shape[0], alpha, topn, window,
                            int(normalize_emb), _ptr(out), C.byref(cnt)))
    return out[:cnt.value]


def dpp_ex(ctx: Context, table: Optional[Table], cand_rows, rel, alpha: float, topn: int, window: int,
           normalize_emb: bool = True, ensure_pos_similarity: bool = True, norm_relevance_score: int = 0,
           hook_emb: Optional[np.ndarray] = None):
    """pg_dpp_ex: DPPSort.KernelMatrix + DPPWithWindow with every option.  table=None → hook embeddings only.
    Returns (picked indices, relevance scores as used)."""
    r = np.ascontiguousarray(rel, dtype=np.float64)
    n = r.shape[0]
    c = np.ascontiguousarray(cand_rows, dtype=np.uint32) if table is not None else None
    h = None if hook_emb is None else np.ascontiguousarray(hook_emb, dtype=np.float64).reshape(n, -1)
    opt = _lib.PgDppOptions(alpha, topn, window, int(normalize_emb), int(ensure_pos_similarity),
                            int(norm_relevance_score), int(table is not None), 0 if h is None else h.shape[1])
    out = np.zeros(max(topn, 1), dtype=np.uint32)
    used = np.zeros(max(n, 1), dtype=np.float64)
    cnt = C.c_uint32()
    _lib.check(ctx.L.pg_dpp_ex(ctx.h, table.h if table is not None else None, _ptr(c) if c is not None else None,
                               _ptr(r), n, C.byref(opt), _ptr(h) if h is not None else None, _ptr(out),
                               C.byref(cnt), _ptr(used)))
    return out[:cnt.value], used[:n]


def ssd(ctx: Context, table: Table, cand_rows, rel, gamma: float, topn: int, window: int,
        normalize_emb: bool = True, ensure_pos_similarity: bool = True, norm_quality_score: int = 0,
        use_ssd_star: bool = False):
    """SSDSort.SSDWithSlidingWindow over candidates given in score-descending order.
    Returns (picked indices, quality scores)."""
    c = np.ascontiguousarray(cand_rows, dtype=np.uint32)
    r = np.ascontiguousarray(rel, dtype=np.float64)
    out = np.zeros(max(c.shape[0], 1), dtype=np.uint32)
    qual = np.zeros(max(c.shape[0], 1), dtype=np.float64)
    cnt = C.c_uint32()
    _lib.check(ctx.L.pg_ssd(ctx.h, table.h, _ptr(c), _ptr(r), c.shape[0], gamma, topn, window,
                            int(normalize_emb), int(ensure_pos_similarity), int(norm_quality_score),
                            int(use_ssd_star), _ptr(out), C.byref(cnt), _ptr(qual)))
    return out[:cnt.value], qual[:c.shape[0]]


def ssd_emb(ctx: Context, emb, rel, gamma: float, topn: int, window: int, normalize_emb: bool = True,
            ensure_pos_similarity: bool = True, norm_quality_score: int = 0, use_ssd_star: bool = False):
    """pg_ssd_emb: pg_ssd over the candidates' own fp32 embeddings [n][dim] (any dim).  Returns (picked indices, quality scores)."""
    e = np.ascontiguousarray(emb, dtype=np.float32)
    r = np.ascontiguousarray(rel, dtype=np.float64)
    n = r.shape[0]
    e = e.reshape(n, -1)
    out = np.zeros(max(n, 1), dtype=np.uint32)
    qual = np.zeros(max(n, 1), dtype=np.float64)
    cnt = C.c_uint32()
    _lib.check(ctx.L.pg_ssd_emb(ctx.h, _ptr(e), e.shape[1], _ptr(r), n, gamma, topn, window, int(normalize_emb),
                                int(ensure_pos_similarity), int(norm_quality_score), int(use_ssd_star), _ptr(out),
                                C.byref(cnt), _ptr(qual)))
    return out[:cnt.value], qual[:n]


F_I32, F_I64, F_F32, F_F64 = 1, 2, 3, 4
_F_NP = {F_I32: np.int32, F_I64: np.int64, F_F32: np.float32, F_F64: np.float64}


class Features:
    """Typed item-feature columns in HBM (pg_features_*): the device form of the reference's per-request
    "context features" (service/rank/algo_data.go:223-306)."""

    def __init__(self, ctx: Context, rows: int):
        self.ctx, self.rows = ctx, rows
        h = C.c_void_p()
        _lib.check(ctx.L.pg_features_create(ctx.h, rows, C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            _lib.check(self.ctx.L.pg_features_destroy(self.ctx.h, self.h))
            self.h = None

    def set_column(self, name: str, dtype: int, values: Optional[np.ndarray] = None, default: float = 0.0):
        v = None
        if values is not None:
            v = np.ascontiguousarray(values, dtype=_F_NP[dtype])
            assert v.shape == (self.rows,)
        _lib.check(self.ctx.L.pg_features_set_column(self.ctx.h, self.h, name.encode(), dtype,
                                                     _ptr(v) if v is not None else None, float(default)))

    def index(self, name: str) -> int:
        return int(self.ctx.L.pg_features_column_index(self.h, name.encode()))

    def _cols(self, names) -> np.ndarray:
        idx = np.asarray([self.index(n) if isinstance(n, str) else int(n) for n in names], dtype=np.int32)
        return idx

    def eval_expr(self, expr: "Expr", rows: np.ndarray) -> np.ndarray:
        """The expression with its variables bound to the columns of their names at `rows`, fp64 (pg_features_eval_dev):
        a numeric `expression` normalizer over item features for a candidate batch."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        d_r = self.ctx.to_device(r)
        d_o = self.ctx.malloc(max(r.shape[0] * 8, 16))
        try:
            _lib.check(self.ctx.L.pg_features_eval_dev(self.ctx.h, self.h, expr.h, d_r, r.shape[0], d_o))
            out = np.zeros(r.shape[0], dtype=np.float64)
            self.ctx.d2h(out, d_o)
        finally:
            self.ctx.free(d_r)
            self.ctx.free(d_o)
        return out

    def gather_i32(self, names, rows: np.ndarray) -> np.ndarray:
        idx = self._cols(names)
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        d_r = self.ctx.to_device(r)
        d_o = self.ctx.malloc(max(r.shape[0] * idx.shape[0] * 4, 16))
        try:                                              # (a refused column must not leak the two buffers)
            _lib.check(self.ctx.L.pg_features_gather_i32_dev(self.ctx.h, self.h, _ptr(idx), idx.shape[0], d_r,
                                                             r.shape[0], d_o))
            out = np.zeros((r.shape[0], idx.shape[0]), dtype=np.int32)
            self.ctx.d2h(out, d_o)
        finally:
            self.ctx.free(d_r)
            self.ctx.free(d_o)
        return out

    def gather_f32(self, names, rows: np.ndarray, scale=None, bias=None) -> np.ndarray:
        idx = self._cols(names)
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
        bi = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        d_r = self.ctx.to_device(r)
        d_o = self.ctx.malloc(max(r.shape[0] * idx.shape[0] * 4, 16))
        _lib.check(self.ctx.L.pg_features_gather_f32_dev(self.ctx.h, self.h, _ptr(idx), idx.shape[0],
                                                         _ptr(sc) if sc is not None else None,
                                                         _ptr(bi) if bi is not None else None, d_r, r.shape[0], d_o))
        out = np.zeros((r.shape[0], idx.shape[0]), dtype=np.float32)
        self.ctx.d2h(out, d_o)
        self.ctx.free(d_r)
        self.ctx.free(d_o)
        return out
