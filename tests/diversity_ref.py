"""DiversityRuleSort as include/pairec_gpu.h defines it: the specification the GPU tests compare with.

Position-based and item by item: nothing is vectorised, no key stands for a value, a rule's match walks the result's tail as
sort/diversity_rule.go:50-92 does.  tests/test_diversity_cpu.py holds it against a literal transcription of the reference's loops
(sort/diversity_rule_sort.go:116-283) and pg_diversity_rules_host against it.

A config is the dict pairec_amd.engine._div_config takes: {"size", "diversity_size", "explore_item_size", "exclude_source_mask",
"rules": [{"dims", "interval", "window", "frequency", "weight"}], "exclusions": [{"positions", "terms": [(column, op, value)]}]}."""
import numpy as np

MAX_N, MAX_RULES, MAX_DIMS, MAX_COLS, MAX_EXCL, MAX_TERMS, MAX_POSITIONS, CHUNK, WAVE = 8192, 8, 4, 16, 8, 4, 64, 1024, 64
GT, GE, LT, LE, EQ, NE = range(6)
NONE = 0xFFFFFFFF

_OPS = {GT: lambda v, c: v > c, GE: lambda v, c: v >= c, LT: lambda v, c: v < c, LE: lambda v, c: v <= c, EQ: lambda v, c: v == c,
        NE: lambda v, c: v != c}


def rule_fails(rule, value, tail_values):
    """diversity_rule.go:50-92 — tail_values: the rule's values of the result so far, in order; the last max(interval, window)
    of them are enough: s >= interval and the window's span read the same from them as from the whole result"""
    s = len(tail_values)
    interval, window, frequency = rule.get("interval", 0), rule.get("window", 0), rule.get("frequency", 0)
    if interval > 0 and s >= interval and tail_values[s - interval:].count(value) == interval:
        return True
    if window > 0 and frequency > 0 and window > frequency and 1 + tail_values[max(0, s - window + 1):].count(value) > frequency:
        return True
    return False


def sort_one(cfg, n, cols, source=None, enable=True):
    """one request: cols[c][i] = column c of the entry at position i (i < n) → the order, a list of n positions"""
    rules, excl = cfg.get("rules", []), cfg.get("exclusions", [])
    if not rules or not enable:
        return list(range(n))
    mask = cfg.get("exclude_source_mask", 0)
    aside = [p for p in range(n) if mask and source is not None and int(source[p]) < 32 and (mask >> int(source[p])) & 1]
    aside_set = set(aside)
    kept = [p for p in range(n) if p not in aside_set]
    m = len(kept)
    if m == 0:
        return list(range(n))

    def value(k, j):                             # rule k's value of kept entry j
        return tuple(int(cols[c][kept[j]]) for c in rules[k]["dims"])

    where = [set(e["positions"]) for e in excl]

    def excluded(position, j):
        return any(position in where[i] and all(_OPS[op](int(cols[c][kept[j]]), v) for c, op, v in e["terms"]) for i, e in enumerate(excl))

    D = cfg.get("size", 0)
    if cfg.get("diversity_size", 0) > 0:
        D = min(cfg["diversity_size"], m)
    explore = cfg.get("explore_item_size", 0)
    has_weight = any(r.get("weight", 0) > 0 for r in rules)
    taken = [False] * m
    first = next((j for j in range(m) if not excluded(1, j)), 0)
    taken[first] = True
    result = [first]
    while len(result) <= D and len(result) != m:
        f, best, best_w, pick = None, None, 0, None
        tails = [[value(k, x) for x in result[-max(r.get("interval", 0), r.get("window", 0), 1):]] for k, r in enumerate(rules)]
        for j in range(m):
            if taken[j] or excluded(len(result) + 1, j):
                continue
            if f is None:
                f = j
            if explore > 0 and j - f >= explore:
                break
            fails = [rule_fails(r, value(k, j), tails[k]) for k, r in enumerate(rules)]
            if not any(fails):
                pick = j
                break
            w = sum(r.get("weight", 0) for r, bad in zip(rules, fails) if not bad) if has_weight else 0
            if best is None or w > best_w:
                best, best_w = j, w
        if pick is None:
            if f is None:
                break
            pick = best
        taken[pick] = True
        result.append(pick)
    return [kept[j] for j in result] + [kept[j] for j in range(m) if not taken[j]] + aside


def diversity_rules(cfg, dims, count=None, source=None, enable=None):
    """dims [n_cols][nq][cap] → order [nq][cap] uint32, UINT32_MAX behind count"""
    dims = np.asarray(dims, dtype=np.int64)
    _, nq, cap = dims.shape
    out = np.full((nq, cap), NONE, np.uint32)
    for q in range(nq):
        n = cap if count is None else min(int(count[q]), cap)
        out[q, :n] = sort_one(cfg, n, dims[:, q, :].tolist(), None if source is None else np.asarray(source[q]).tolist(), True if enable is None else bool(enable[q]))
    return out
