"""TrafficControlSort's macro control (include/pairec_gpu.h "TrafficControlSort") restated in plain Python, one
entry at a time, from the reference's Go (sort/traffic_control_sort.go: macroControl :204-364, computeDeltaRank :555-589, tanh /
sigmoid :942-960, the closing loop and ItemRankSlice :160-181, :924-934) and not from the library's C++.  Python floats are IEEE
doubles and every operation below is one rounding, as in Go; Go's int is modelled by goint and by wrapping to 64 bits after every
integer operation.  The four tables are arguments: the tests hand over the library's own (pg_traffic_table), so that two libms
need not agree in the last bit.  Where the reference walks a Go map (random order) the targets go in ascending index, and where its
comparator is no order (NaN positions) NaN sorts last: both are the header's definitions."""
import math

import numpy as np

PERCENT, QUANTITY = 1, 2
INT64_MIN = -(1 << 63)
NAN_BITS = 0x7FF8000000000000
EMPTY = 0xFFFFFFFF


def goint(x: float) -> int:
    """Go's int(float64) on amd64 (CVTTSD2SQ): truncation inside (-2^63, 2^63), the "integer indefinite" INT64_MIN otherwise"""
    if x != x or not (-9223372036854775808.0 < x < 9223372036854775808.0):
        return INT64_MIN
    return int(x)          # Python's int() truncates toward zero


def wrap(v: int) -> int:
    """an int64 after an operation that may have overflowed"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def make_tables():
    """the reference's init() (:45-66) with Python's libm: what the library's tables are held against (to 1 ulp)"""
    pos = [math.exp(-0.01 * float(i)) for i in range(500)]
    exp = [math.exp(float(i) / 1000.0) for i in range(1000)]
    tanh = [math.tanh(float(i) / 1000.0) for i in range(3000)]
    sig = [1.0 / (1.0 + math.exp(10 - (float(i) / 1000.0 + 5.0))) for i in range(10000)]
    return pos, exp, tanh, sig


def _div(a: float, b: float) -> float:
    """Go's float64 division: a zero divisor gives +-Inf or NaN, it does not panic"""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -math.inf if neg else math.inf
    return a / b


def _mul(a: float, b: float) -> float:
    return float(np.float64(a) * np.float64(b))       # (numpy: inf * 0 = NaN without an exception, overflow to inf)


def _add(a: float, b: float) -> float:
    return float(np.float64(a) + np.float64(b))


class Tables:
    def __init__(self, pos, exp, tanh, sig):
        self.pos, self.exp, self.tanh, self.sig = [list(map(float, t)) for t in (pos, exp, tanh, sig)]
        assert (len(self.pos), len(self.exp), len(self.tanh), len(self.sig)) == (500, 1000, 3000, 10000)

    def tanh_(self, x: float) -> float:                 # :942-950
        idx = goint(_mul(x, 1000.0))
        if idx < 0:
            idx = 0
        elif idx >= 3000:
            idx = 2999
        return self.tanh[idx]

    def sigmoid(self, x: float, rho: float) -> float:   # :952-960
        idx = wrap(goint(_mul(_mul(rho, x), 1000.0)) - 5000)
        if idx < 0:
            idx = 0
        elif idx >= 10000:
            return 1.0
        return self.sig[idx]


def request(tables: Tables, targets, ctx_size: int, page_no: int, gamma: float, beta: float, eta: float, scores, members, alphas):
    """one request: scores / members in LIST order (n entries), alphas [T], targets [(target_id, control_type)] →
    (order: list indices in their new order, control_id [n], new_pos [n])"""
    n, T = len(scores), len(targets)
    with np.errstate(all="ignore"):
        control = [i + 1 for i in range(n)]                # :115-118
        origin = [i + 1 for i in range(n)]
        delta_rank = [0.0] * n
        alpha_map = {t: float(alphas[t]) for t in range(T)}
        if n and T and any(a != 0 for a in alpha_map.values()):      # :131-135, :208-211
            item_scores = [0.0] * n
            total, max_score = 0.0, 0.0
            target_score = {}
            for i in range(n):                              # :222-253
                score = float(scores[i])
                if score == 0.0:
                    score = 1e-8
                if i == 0:
                    max_score = score
                    item_scores[0] = math.e
                else:
                    v = _div(score, max_score)
                    idx = goint(_mul(v, 1000.0))
                    if idx < 0:
                        idx = 0
                    if idx >= 1000:
                        idx = 999
                    item_scores[i] = tables.exp[idx]
                pos_weight = 0.006737946999
                if i < 500:
                    pos_weight = tables.pos[i]
                score = _mul(score, pos_weight)
                total = _add(total, score)
                for t in range(T):
                    if alpha_map[t] != 0 and (int(members[i]) >> t) & 1:
                        target_score[t] = _add(target_score.get(t, 0.0), score)
            for t in list(target_score):                    # :254-256
                target_score[t] = _div(target_score[t], total)
            for t in range(T):                              # :284-291
                alpha = alpha_map[t]
                if alpha > 0:
                    w = target_score.get(t, 0.0)
                    rho = _add(1.0, _mul(gamma, tables.tanh_(_mul(beta, w))))
                    alpha_map[t] = _mul(alpha, rho)
            for i in range(n):                              # :332-356
                final = 0.0
                for t in range(T):
                    if not (int(members[i]) >> t) & 1:
                        continue
                    alpha = alpha_map[t]
                    if alpha == 0:
                        continue
                    # computeDeltaRank (:555-589)
                    w = target_score.get(t, 0.0)
                    delta = alpha
                    if alpha < 0.0:
                        rho = _mul(eta, _add(1.0, -tables.tanh_(w)))
                        delta = _mul(delta, tables.sigmoid(float(i), rho))
                    else:
                        delta = _mul(delta, item_scores[i])
                        start = ctx_size
                        if page_no > 1:
                            multiple = _mul(_add(w, -0.3), 10.0)
                            start = wrap(start + goint(_mul(multiple, float(ctx_size))))
                        if i > start and delta >= 1.0:
                            tid, ty = targets[t]
                            if ty == PERCENT:
                                control[i] = -tid
                            elif control[i] > 0:
                                control[i] = 0
                    final = _add(final, delta)
                if final != 0.0:
                    delta_rank[i] = final
                    if control[i] == 0 and final < 1.0:
                        control[i] = origin[i]
        new_pos = [0.0] * n
        for i in range(n):                                  # :160-180
            if delta_rank[i] != 0.0:
                new_pos[i] = float(np.float64(i + 1) - np.float64(delta_rank[i]))
                if new_pos[i] != new_pos[i]:
                    new_pos[i] = float(np.uint64(NAN_BITS).view(np.float64))      # (step 7: one NaN)
            else:
                new_pos[i] = float(i + 1)

    def key(i):                                             # ItemRankSlice (:924-934); NaN behind every number (the header's step 8)
        p = new_pos[i]
        return (1, 0.0, origin[i]) if p != p else (0, p, origin[i])
    order = sorted(range(n), key=key)
    return order, control, new_pos


def traffic_sort(tables: Tables, targets, ctx_size: int, nq: int, cap: int, score=None, member=None, order=None, count=None, alpha=None,
                 page_no: int = 1, gamma: float = 1.0, beta: float = 1.0, eta: float = 1.6):
    """the whole call → (out_order [nq][cap] u32, out_count [nq] u32, control_id [nq][cap] i32, new_pos [nq][cap] f64), by element
    as the header's Outputs state them.  A list entry whose order value is >= cap leaves the list first (the device's rule)."""
    T = len(targets)
    out = np.full((nq, cap), EMPTY, np.uint32)
    out_count = np.zeros(nq, np.uint32)
    cid = np.zeros((nq, cap), np.int32)
    pos = np.full((nq, cap), np.uint64(NAN_BITS).view(np.float64), np.float64)
    score = None if score is None else np.asarray(score, np.float64).reshape(nq, cap)
    member = None if member is None else np.asarray(member, np.uint8).reshape(nq, cap)
    alpha = None if alpha is None else np.asarray(alpha, np.float64).reshape(nq, T)
    order = None if order is None else np.asarray(order, np.uint32).reshape(nq, cap)
    for q in range(nq):
        n = cap if count is None else min(int(count[q]), cap)
        elems = [int(order[q][j]) if order is not None else j for j in range(n)]
        elems = [e for e in elems if e < cap]
        sc = [score[q][e] for e in elems] if T else [0.0] * len(elems)
        mem = [member[q][e] for e in elems] if T else [0] * len(elems)
        o, c, p = request(tables, list(targets), ctx_size, page_no, gamma, beta, eta, sc, mem, alpha[q] if T else [])
        out_count[q] = len(elems)
        for k, i in enumerate(o):
            out[q][k] = elems[i]
        for i, e in enumerate(elems):
            cid[q][e] = np.int64(c[i]).astype(np.int32)
            pos[q][e] = p[i]
    return out, out_count, cid, pos
