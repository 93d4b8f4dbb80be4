"""DiversityAdjustCountFilter (filter/diversity_adjust_count_filter.go:75-143) restated in numpy and plain Python, sharing
nothing with the library: expression TREES evaluated with govaluate's three-valued rules (a value, or an error), the cut as
include/pairec_gpu.h defines it, and — separately — an item-by-item transcription of the Go loop (:115-140) that the
restatement is held against.  Random tests generate trees, render them to govaluate text for the library and evaluate the
tree here: there is no second parser.

A tree is a tuple:
    ("num", v)  ("col", name)  ("score",)  ("neg", x)  ("round", x)  ("bin", op, l, r)   op in + - * / % **
    ("cmp", op, l, r)  op in == != > >= < <=     ("in", x, [constants])     ("and", l, r)  ("or", l, r)  ("not", x)
    ("rn_eq", lit)  ("rn_ne", lit)  ("rn_in", [lits])                        recall_name against string literals
"""
import math

import numpy as np

FIX, ACCUMULATE = 0, 1
PAD_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_BITS = np.uint64(0x7FF8000000000000)
MAX_CLASSES, MAX_CAP, MAX_OPS, MAX_DEPTH, MAX_LIST, MAX_COLS = 8, 16384, 64, 8, 64, 16


class _Err:
    def __repr__(self):
        return "ERR"


ERR = _Err()       # govaluate's evaluation error ("No parameter found")


def _go_round(x):
    """math.Round: half away from zero"""
    if math.isnan(x) or math.isinf(x):
        return x
    t = float(math.trunc(x))
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return math.copysign(t, x)


def _arith(op, l, r):
    l, r = np.float64(l), np.float64(r)
    with np.errstate(all="ignore"):
        if op == "+":
            return float(l + r)
        if op == "-":
            return float(l - r)
        if op == "*":
            return float(l * r)
        if op == "/":
            return float(l / r)
        if op == "%":
            return float(np.fmod(l, r))
        if op == "**":
            if r == 2.0:
                return float(l * l)          # (what Go's math.Pow gives for an exponent of 2, bit for bit)
            return float(np.power(l, r))     # (other exponents: not used where bits decide)
    raise ValueError(op)


def _compare(op, l, r):
    return {"==": l == r, "!=": l != r, ">": l > r, ">=": l >= r, "<": l < r, "<=": l <= r}[op]


def evaluate(t, cols, score, recall_name):
    """the tree on one candidate → float, bool or ERR.  cols: {name: float} or None for a candidate outside the store (every
    declared column missing); recall_name: the source's name, None for a source that has none"""
    k = t[0]
    if k == "num":
        return float(t[1])
    if k == "col":
        return ERR if cols is None else float(cols[t[1]])
    if k == "score":
        return float(score)
    if k in ("neg", "round", "not"):
        x = evaluate(t[1], cols, score, recall_name)
        if x is ERR:
            return ERR
        return -x if k == "neg" else _go_round(x) if k == "round" else (not x)
    if k == "bin" or k == "cmp":
        l = evaluate(t[2], cols, score, recall_name)
        r = evaluate(t[3], cols, score, recall_name)
        if l is ERR or r is ERR:
            return ERR
        return _arith(t[1], l, r) if k == "bin" else bool(_compare(t[1], l, r))
    if k == "in":
        x = evaluate(t[1], cols, score, recall_name)
        return ERR if x is ERR else any(x == float(c) for c in t[2])
    if k == "and" or k == "or":
        l = evaluate(t[1], cols, score, recall_name)
        if l is ERR:
            return ERR
        if l == (k == "or"):                 # false && …, true || …: the right side is not looked at
            return l
        return evaluate(t[2], cols, score, recall_name)
    if k == "rn_eq":
        return recall_name is not None and recall_name == t[1]
    if k == "rn_ne":
        return not (recall_name is not None and recall_name == t[1])
    if k == "rn_in":
        return recall_name is not None and recall_name in t[1]
    raise ValueError(k)


def _num_text(v):
    v = float(v)
    s = repr(abs(v))
    assert "e" not in s and "n" not in s, v      # digits and '.' only
    return ("-" if math.copysign(1.0, v) < 0 else "") + (s[:-2] if s.endswith(".0") else s)


def render(t):
    """the tree as govaluate text, every composite operand in parentheses (precedence is pinned by hand-written strings)"""
    k = t[0]
    if k == "num":
        return _num_text(t[1])
    if k == "col":
        return t[1]
    if k == "score":
        return "recall_score"
    if k == "neg":
        return "-(%s)" % render(t[1])
    if k == "round":
        return "round(%s)" % render(t[1])
    if k == "not":
        return "!(%s)" % render(t[1])
    if k == "bin" or k == "cmp":
        return "(%s) %s (%s)" % (render(t[2]), t[1], render(t[3]))
    if k == "in":
        return "(%s) in (%s)" % (render(t[1]), ", ".join(_num_text(c) for c in t[2]))
    if k == "and" or k == "or":
        return "(%s) %s (%s)" % (render(t[1]), "&&" if k == "and" else "||", render(t[2]))
    if k == "rn_eq":
        return "recall_name == '%s'" % t[1]
    if k == "rn_ne":
        return 'recall_name != "%s"' % t[1]
    if k == "rn_in":
        return "recall_name in (%s)" % ", ".join("'%s'" % s for s in t[1])
    raise ValueError(k)


def shape(t):
    """(operations, stack depth) of the tree's postfix program"""
    k = t[0]
    if k in ("num", "col", "score", "rn_eq", "rn_in"):
        return 1, 1
    if k == "rn_ne":
        return 2, 1
    if k in ("neg", "round", "not"):
        n, d = shape(t[1])
        return n + 1, d
    if k == "in":
        n, d = shape(t[1])
        return n + 1, d
    a, b = (t[2], t[3]) if k in ("bin", "cmp") else (t[1], t[2])
    (na, da), (nb, db) = shape(a), shape(b)
    return na + nb + 1, max(da, db + 1)


def random_number_tree(rng, names, depth):
    r = rng.random()
    if depth == 0 or r < 0.3:
        pick = rng.integers(0, 10)
        if pick < 6 and names:
            return ("col", names[rng.integers(0, len(names))])
        if pick < 7:
            return ("score",)
        return ("num", float(rng.choice([0, 1, 2, 3, -1, -2, 0.5, 2.5, 7, 100, 0.1])))
    if r < 0.4:
        return ("neg", random_number_tree(rng, names, depth - 1))
    if r < 0.45:
        return ("round", random_number_tree(rng, names, depth - 1))
    op = ["+", "-", "*", "/", "%"][rng.integers(0, 5)]
    return ("bin", op, random_number_tree(rng, names, depth - 1), random_number_tree(rng, names, depth - 1))


def random_bool_tree(rng, names, recalls, depth):
    r = rng.random()
    if depth == 0 or r < 0.35:
        pick = rng.integers(0, 10)
        if pick < 6:
            op = ["==", "!=", ">", ">=", "<", "<="][rng.integers(0, 6)]
            return ("cmp", op, random_number_tree(rng, names, 1), random_number_tree(rng, names, 1))
        if pick < 7:
            n = int(rng.integers(2, 5))
            return ("in", random_number_tree(rng, names, 1), [float(v) for v in rng.integers(-2, 4, n)])
        lits = list(recalls) + ["nobody"]
        if pick < 8:
            return ("rn_eq", lits[rng.integers(0, len(lits))])
        if pick < 9:
            return ("rn_ne", lits[rng.integers(0, len(lits))])
        return ("rn_in", [lits[j] for j in rng.choice(len(lits), 2, replace=False)])
    if r < 0.5:
        return ("not", random_bool_tree(rng, names, recalls, depth - 1))
    return ("and" if r < 0.75 else "or", random_bool_tree(rng, names, recalls, depth - 1), random_bool_tree(rng, names, recalls, depth - 1))


def masks(trees, n, cols, item_in, score, source, recall_names):
    """bit c of out[i] = tree c is true (not an error) on candidate i.  cols: {name: [n] array}, item_in [n] or None, source [n]
    or None"""
    out = np.zeros(n, np.uint8)
    names = list(cols)
    vals = {k: [float(x) for x in np.asarray(v).reshape(-1)] for k, v in cols.items()}      # float64(value), as the columns are read
    for i in range(n):
        inside = item_in is None or bool(item_in[i])
        c = {k: vals[k][i] for k in names} if inside else None
        s = None if source is None else int(source[i])
        rn = recall_names[s] if s is not None and s < len(recall_names) else None
        m = 0
        for b, t in enumerate(trees):
            if evaluate(t, c, float(score[i]), rn) is True:
                m |= 1 << b
        out[i] = m
    return out


def score_order(real, score):
    """pg_sort_scores_dev's order of the positions `real`: descending, -0.0 equals +0.0, NaN last, ties keep input position"""
    return sorted(real, key=lambda p: (1, 0.0) if math.isnan(score[p]) else (0, -float(score[p])))


def out_cap(rules, cap):
    fix = sum(c for t, c in rules if t == FIX)
    acc = max([c for t, c in rules if t == ACCUMULATE], default=0)
    return min(cap, fix + acc)


def cut_positions(rules, rows, score, count, mask):
    """the definition: one request's arrays [cap] → the input positions kept, in output order.  rules: [(type, count)]"""
    cap = len(rows)
    n_valid = cap if count is None else min(int(count), cap)
    order = score_order([p for p in range(n_valid) if rows[p] != PAD_ROW], score)
    members = [[p for p in order if (int(mask[p]) >> c) & 1] for c in range(len(rules))]
    taken, out, acc = set(), [], 0
    for c, (type_, cnt) in enumerate(rules):
        limit = cnt if type_ == FIX else max(0, cnt - acc)
        picks = [p for p in members[c][:limit] if p not in taken]
        taken.update(picks)
        out += picks
        if type_ == ACCUMULATE:
            acc += len(picks)
    return out


def cut_positions_go(rules, rows, score, count, mask):
    """the Go loop (:115-140) item by item over the same score order"""
    cap = len(rows)
    n_valid = cap if count is None else min(int(count), cap)
    items = score_order([p for p in range(n_valid) if rows[p] != PAD_ROW], score)
    recall_to_items = {}
    for p in items:                                         # :92-103
        for cid in range(len(rules)):
            if (int(mask[p]) >> cid) & 1:
                recall_to_items.setdefault(cid, []).append(p)
    new_items, duplicate, accumulator = [], {}, 0
    for cid, (type_, cnt) in enumerate(rules):
        recall_items = recall_to_items.get(cid, [])
        if type_ == FIX:
            i = 0
            while i < len(recall_items) and i < cnt:
                if recall_items[i] in duplicate:
                    i += 1
                    continue
                new_items.append(recall_items[i])
                duplicate[recall_items[i]] = True
                i += 1
        else:
            c = cnt - accumulator
            i = 0
            while i < len(recall_items) and i < c:
                if recall_items[i] in duplicate:
                    i += 1
                    continue
                new_items.append(recall_items[i])
                duplicate[recall_items[i]] = True
                accumulator += 1
                i += 1
    return new_items


def classcut(rules, rows, score, mask, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """the whole answer on [nq][cap] arrays (mask [nq][cap] uint8: the class bits) → (rows, score, source, planes_f64,
    source_mask, planes_f32, count) at [nq][out_cap], None where the input is None; padding as the trim's"""
    nq, cap = rows.shape
    w = out_cap(rules, cap)
    o_rows = np.full((nq, w), PAD_ROW, np.uint64)
    o_score = np.full((nq, w), -np.inf, np.float64)
    o_src = None if source is None else np.full((nq, w), 0xFF, np.uint8)
    o_p64 = None if planes_f64 is None else np.full((planes_f64.shape[0], nq, w), NAN_BITS, np.uint64).view(np.float64)
    o_mask = None if source_mask is None else np.zeros((nq, w), np.uint32)
    o_p32 = None if planes_f32 is None else np.zeros((planes_f32.shape[0], nq, w), np.float32)
    o_cnt = np.zeros(nq, np.uint32)
    for q in range(nq):
        keep = cut_positions(rules, rows[q], score[q], None if count is None else count[q], mask[q])
        assert len(keep) <= w
        k = np.asarray(keep, dtype=np.int64)
        n = len(keep)
        o_cnt[q] = n
        o_rows[q, :n] = rows[q, k]
        o_score[q, :n].view(np.uint64)[:] = score[q, k].view(np.uint64)
        if o_src is not None:
            o_src[q, :n] = source[q, k]
        if o_p64 is not None:
            o_p64[:, q, :n].view(np.uint64)[:] = planes_f64[:, q, k].view(np.uint64)
        if o_mask is not None:
            o_mask[q, :n] = source_mask[q, k]
        if o_p32 is not None:
            o_p32[:, q, :n].view(np.uint32)[:] = planes_f32[:, q, k].view(np.uint32)
    return o_rows, o_score, o_src, o_p64, o_mask, o_p32, o_cnt


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
