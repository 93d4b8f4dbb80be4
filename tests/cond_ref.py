"""A sequential restatement of the compiled condition set's specification (include/pairec_gpu.h: pg_cond_*) over
integer-coded columns: FilterParam matching, BoostScoreSort's walk, ItemStateFilter's order-preserving keep, and the govaluate
arithmetic subset.  Plain Python, one candidate at a time; tests hold it against a literal transcription of the Go code
(test_cond_cpu.py) and hold the host functions and the kernels against it.

A config is the reference's JSON: [{"Name", "Domain", "Operator", "Type", "Value", "Configs"}]; string values are dictionary ids
already.  cols: {name: array}, candidate-aligned (cols[name][i] belongs to candidate i) with int / float dtypes; item_in[i] False:
the candidate's row is outside the store (every item property missing); user: {name: value}, a missing name = an absent slot."""
import math
import struct

import numpy as np

from oracle import oracle as o

ORDERED = {"greater": lambda a, b: a > b, "greaterThan": lambda a, b: a >= b, "less": lambda a, b: a < b, "lessThan": lambda a, b: a <= b}
# the answer when the left property is missing / when a user.x or item.x right-hand side is missing (float, integer types)
LEFT_MISSING = {"equal": False, "not_equal": True, "in": False, "not_in": False, "greater": False, "greaterThan": False, "less": False,
                "lessThan": False}
USER_RHS_MISSING = {"equal": False, "not_equal": True, "greater": False, "greaterThan": False, "less": False, "lessThan": False}
ITEM_RHS_MISSING = {"equal": (False, False), "not_equal": (True, True), "greater": (True, False), "greaterThan": (True, False),
                    "less": (True, False), "lessThan": (True, False)}
TYPES_LISTED = {"equal": ("string", "int", "int64"), "not_equal": ("string", "int", "int64"), "in": ("string", "int"), "not_in": ("string", "int"),
                "greater": ("float", "int", "int64"), "greaterThan": ("float", "int", "int64"), "less": ("float", "int", "int64"),
                "lessThan": ("float", "int", "int64")}


def _value(raw, type_):
    return float(raw) if type_ == "float" else int(raw)


def term(cfg, i, cols, item_in, user):
    op, type_, name = cfg["Operator"], cfg.get("Type", ""), cfg.get("Name", "")
    domain = cfg.get("Domain") or "item"
    if op == "bool":
        kids = [term(c, i, cols, item_in, user) for c in cfg.get("Configs", ())]
        return any(kids) if (type_ or "").lower() in ("", "or") else all(kids)
    if domain == "user":
        present, raw = name in user, user.get(name)
    else:
        present, raw = bool(item_in[i]), (cols[name][i] if item_in[i] else None)
    if op == "is_null":
        return not present
    if op == "is_not_null":
        return present
    if not present:
        return LEFT_MISSING[op]
    if type_ not in TYPES_LISTED[op]:
        return False
    if op in ("in", "not_in"):
        found = int(raw) in [int(v) for v in cfg["Value"]]
        return found if op == "in" else not found
    v = cfg.get("Value")
    if isinstance(v, str) and v.startswith("user."):
        if v[5:] not in user:
            return USER_RHS_MISSING[op]
        right = user[v[5:]]
    elif isinstance(v, str) and v.startswith("item."):
        if not item_in[i]:
            return ITEM_RHS_MISSING[op][0 if type_ == "float" else 1]
        right = cols[v[5:]][i]
    else:
        right = v
    a, b = _value(raw, type_), _value(right, type_)
    if op == "equal":
        return a == b
    if op == "not_equal":
        return a != b
    return ORDERED[op](a, b)


def match(conditions, i, cols, item_in, user):
    return all(term(c, i, cols, item_in, user) for c in conditions)


# ---- the govaluate arithmetic subset ------------------------------------------------------------------------------------------
class _P:
    def __init__(self, s):
        self.s, self.i = s, 0

    def ws(self):
        while self.i < len(self.s) and self.s[self.i] in " \t\r\n":
            self.i += 1

    def peek(self, t):
        self.ws()
        return self.s.startswith(t, self.i)

    def add(self):
        l = self.mul()
        while True:
            self.ws()
            if self.i < len(self.s) and self.s[self.i] in "+-":
                op = self.s[self.i]
                self.i += 1
                r = self.mul()
                l = (op, l, r)
            else:
                return l

    def mul(self):
        l = self.power()
        while True:
            self.ws()
            if self.i < len(self.s) and self.s[self.i] in "*/%" and not self.s.startswith("**", self.i):
                op = self.s[self.i]
                self.i += 1
                r = self.power()
                l = (op, l, r)
            else:
                return l

    def power(self):
        l = self.prefix()
        if self.peek("**"):
            self.i += 2
            l = ("**", l, self.prefix())
        return l

    def prefix(self):
        self.ws()
        if self.s[self.i] == "-":
            self.i += 1
            return ("neg", self.prefix())
        return self.value()

    def value(self):
        self.ws()
        c = self.s[self.i]
        if c == "(":
            self.i += 1
            e = self.add()
            self.ws()
            assert self.s[self.i] == ")"
            self.i += 1
            return e
        if c == "[":
            j = self.s.index("]", self.i)
            name = self.s[self.i + 1:j]
            self.i = j + 1
            return ("var", name)
        if c.isdigit() or c == ".":
            j = self.i
            while j < len(self.s) and (self.s[j].isdigit() or self.s[j] == "."):
                j += 1
            v = float(self.s[self.i:j])
            self.i = j
            return ("num", v)
        j = self.i
        while j < len(self.s) and (self.s[j].isalnum() or self.s[j] == "_"):
            j += 1
        name = self.s[self.i:j]
        self.i = j
        if self.peek("("):
            assert name == "round"
            self.i += 1
            args = [self.add()]
            if self.peek(","):
                self.i += 1
                args.append(self.add())
            assert self.peek(")")
            self.i += 1
            return ("round", *args)
        return ("var", name)


def expr_parse(source):
    p = _P(source)
    e = p.add()
    p.ws()
    assert p.i == len(source), source
    return e


def expr_vars(e, out=None):
    out = [] if out is None else out
    if e[0] == "var":
        if e[1] not in out:
            out.append(e[1])
    elif e[0] != "num":
        for k in e[1:]:
            expr_vars(k, out)
    return out


def _div(a, b):
    if b == 0.0:
        if a != a:
            return a                                         # a NaN operand travels, payload and all
        return math.nan if a == 0.0 else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def expr_eval(e, env):
    """env: {name: float}; KeyError where govaluate reports "No parameter found" """
    k = e[0]
    if k == "num":
        return e[1]
    if k == "var":
        return float(env[e[1]])
    if k == "neg":
        return -expr_eval(e[1], env)
    if k == "round":
        x = expr_eval(e[1], env)
        if len(e) == 2:
            return _go_round(x)
        m = o.go_pow(10.0, expr_eval(e[2], env))
        t = x * m
        return _div(float(np.trunc(np.float64(t))), m)                # (math.Trunc keeps the sign of a zero)
    a, b = expr_eval(e[1], env), expr_eval(e[2], env)
    if k == "+":
        return a + b
    if k == "-":
        return a - b
    if k == "*":
        return a * b
    if k == "/":
        return _div(a, b)
    if k == "%":
        if a != a or b != b:
            return a + b                                     # a NaN operand travels, payload and all
        return math.fmod(a, b) if (b != 0.0 and math.isfinite(a)) else math.nan                 # math.Mod
    return o.go_pow(a, b)


def _go_round(x):
    """math.Round: half away from zero"""
    if not math.isfinite(x):
        return x
    t = math.trunc(x)
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return math.copysign(t, x) if t == 0 else t


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def score_bits(a):
    """scores as 64-bit patterns for comparison.  One pattern is folded: the default quiet NaN an invalid operation GENERATES is
    0xFFF8000000000000 on x86 and 0x7FF8000000000000 on gfx950 and in Python's math.nan — IEEE 754 leaves its sign to the
    platform — so the two compare equal.  Every other NaN (a payload an expression carried through) and every number compares
    bit for bit."""
    a = np.ascontiguousarray(a)
    u = (a.view(np.uint64) if a.dtype != np.uint64 else a).copy()
    u[u == np.uint64(0xFFF8000000000000)] = np.uint64(0x7FF8000000000000)
    return u


# ---- the two stages -------------------------------------------------------------------------------------------------------------
def boost(rules, filter_all, score, cols, item_in, user):
    """rules: [{"Conditions", "Expression"}] → (scores [n] fp64, last matching rule [n] uint8, 0xFF none)"""
    n = len(score)
    out, rule = np.array(score, dtype=np.float64), np.full(n, 0xFF, dtype=np.uint8)
    parsed = [expr_parse(r["Expression"]) for r in rules]
    for i in range(n):
        for r, ru in enumerate(rules):
            if not match(ru["Conditions"], i, cols, item_in, user):
                continue
            env = {"score": float(out[i])}
            ok = True
            for v in expr_vars(parsed[r]):
                if v != "score":
                    if not item_in[i]:
                        ok = False
                    else:
                        env[v] = float(cols[v][i])
            if ok:
                out[i] = expr_eval(parsed[r], env)
            rule[i] = r
            if not filter_all:
                break
    return out, rule


def gather(store, store_rows, rows):
    """candidate-aligned views of a store's columns for one request's rows: (cols, item_in)"""
    rows = np.asarray(rows, dtype=np.uint64)
    inside = rows < np.uint64(store_rows)
    idx = np.where(inside, rows, 0).astype(np.int64)
    return {k: v[idx] for k, v in store.items()}, inside


def item_state_filter(conditions, store, store_rows, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None,
                      users=None, keep=None):
    """[nq][cap] inputs as pg_fanin_merge_dev leaves them → (rows, score, source, planes_f64, source_mask, planes_f32, count) as
    Context.item_state_filter returns them.  keep [nq][cap]: the candidates' matches if the caller has them already (from a table
    of match() over the store's rows); padding is dropped whatever keep says."""
    rows = np.asarray(rows, dtype=np.uint64)
    nq, cap = rows.shape
    PAD, NAN = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x7FF8000000000000)
    sb = np.ascontiguousarray(score, dtype=np.float64).view(np.uint64)
    o_rows, o_score = np.full((nq, cap), PAD, dtype=np.uint64), np.full((nq, cap), NAN, dtype=np.uint64)
    o_src = None if source is None else np.full((nq, cap), 0xFF, dtype=np.uint8)
    o_mask = None if source_mask is None else np.zeros((nq, cap), dtype=np.uint32)
    p64 = None if planes_f64 is None else np.ascontiguousarray(planes_f64, dtype=np.float64).view(np.uint64)
    p32 = None if planes_f32 is None else np.ascontiguousarray(planes_f32, dtype=np.float32).view(np.uint32)
    o_p64 = None if p64 is None else np.full(p64.shape, NAN, dtype=np.uint64)
    o_p32 = None if p32 is None else np.zeros(p32.shape, dtype=np.uint32)
    o_cnt = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        if keep is None:
            cols, inside = gather(store, store_rows, rows[q])
            user = {} if users is None or users[q] is None else users[q]
        k = 0
        for i in range(n_valid):
            if rows[q, i] == PAD:
                continue
            if not (keep[q, i] if keep is not None else match(conditions, i, cols, inside, user)):
                continue
            o_rows[q, k], o_score[q, k] = rows[q, i], sb[q, i]
            if o_src is not None:
                o_src[q, k] = source[q][i]
            if o_mask is not None:
                o_mask[q, k] = source_mask[q][i]
            if o_p64 is not None:
                o_p64[:, q, k] = p64[:, q, i]
            if o_p32 is not None:
                o_p32[:, q, k] = p32[:, q, i]
            k += 1
        o_cnt[q] = k
    return (o_rows, o_score.view(np.float64), o_src, None if o_p64 is None else o_p64.view(np.float64), o_mask,
            None if o_p32 is None else o_p32.view(np.float32), o_cnt)


def boost_requests(rules, filter_all, store, store_rows, rows, score, count=None, users=None):
    """[nq][cap] → (score bits [nq][cap] uint64, rule [nq][cap] uint8); padding keeps its bits and gets 0xFF"""
    rows = np.asarray(rows, dtype=np.uint64)
    nq, cap = rows.shape
    PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
    out = np.ascontiguousarray(score, dtype=np.float64).copy()
    rule = np.full((nq, cap), 0xFF, dtype=np.uint8)
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        live = np.array([i for i in range(n_valid) if rows[q, i] != PAD], dtype=np.int64)
        if live.size == 0:
            continue
        cols, inside = gather(store, store_rows, rows[q, live])
        user = {} if users is None or users[q] is None else users[q]
        s, r = boost(rules, filter_all, out[q, live], cols, inside, user)
        # (assignment through views keeps bit patterns: numpy copies doubles)
        out[q, live], rule[q, live] = s, r
    return out.view(np.uint64), rule
