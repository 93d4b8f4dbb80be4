"""CPU restatement of RealTimeU2IRecall's specification (include/pairec_gpu.h, "RealTimeU2IRecall on the device"):
sequential loops over Python floats, literally.  No GPU, no library.

    go_exp              Go's pure math.Exp (math/exp.go), operation for operation; Python floats never fuse a product into a sum
    parse_pairs         EventWeight / EventPlayTime as NewRealtimeUser2ItemBaseDao reads them
    compile_expression  the weight expression: govaluate's arithmetic subset, the function exp, the variables currentTime / eventTime
    triggers            GetTriggerInfos: drop, weigh, combine per item in event order, order, cut
    expand              ListItemsByUser's expansion: the largest sim * prefer term of an item, found in the order given
"""
import math
import re
import struct

import numpy as np

from cf_ref import SimLists  # noqa: F401  (the similarity table on the host)

U32MAX = 0xFFFFFFFF
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_TRIGGERS = 256

LN2HI = 6.93147180369123816490e-01
LN2LO = 1.90821492927058770002e-10
LOG2E = 1.44269504088896338700e+00
OVERFLOW = 7.09782712893383973096e+02
UNDERFLOW = -7.45133219101941108420e+02
NEAR_ZERO = 1.0 / (1 << 28)
P1 = 1.66666666666666657415e-01
P2 = -2.77777777770155933842e-03
P3 = 6.61375632143793436117e-05
P4 = -1.65339022054652515390e-06
P5 = 4.13813679705723846039e-08


def go_exp(x):
    if x != x or x == math.inf:
        return x
    if x == -math.inf:
        return 0.0
    if x > OVERFLOW:
        return math.inf
    if x < UNDERFLOW:
        return 0.0
    if -NEAR_ZERO < x < NEAR_ZERO:
        return 1.0 + x
    k = int(LOG2E * x - 0.5) if x < 0 else int(LOG2E * x + 0.5)         # int() truncates, as Go's does
    hi = x - float(k) * LN2HI
    lo = float(k) * LN2LO
    r = hi - lo
    t = r * r
    c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    try:
        return math.ldexp(y, k)                                         # one rounding, in the subnormal range too
    except OverflowError:
        return math.inf


# ---- the config strings ---------------------------------------------------------------------------------------------------------------
_DECIMAL = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\Z")


def parse_float(s):
    """strconv.ParseFloat(s, 64) → the number, or None where Go reports an error (decimal forms, inf / infinity / nan)"""
    body = s[1:] if s[:1] in ("+", "-") else s
    if body.lower() in ("inf", "infinity"):
        return -math.inf if s[:1] == "-" else math.inf
    if s.lower() == "nan":
        return math.nan
    if not _DECIMAL.match(s):
        return None
    v = float(s)
    return None if math.isinf(v) else v                                 # ErrRange


def parse_pairs(s):
    """"click:1;buy:3.5" → {name: number}; None where a non-empty string yields no pair"""
    out = {}
    for piece in s.split(";"):
        parts = piece.split(":")
        if len(parts) != 2:
            continue
        v = parse_float(parts[1])
        if v is None:
            continue
        out[parts[0]] = v
    return out


# ---- the weight expression -------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    pass


_TOKEN = re.compile(r"\s*(\*\*|[-+*/%(),]|\d+\.?\d*|\.\d+|[A-Za-z_][A-Za-z_0-9]*|\S)")


def compile_expression(src):
    """→ f(currentTime, eventTime); precedence  + -  <  * / %  <  **  <  prefix -  <  value (the engine's govaluate subset)"""
    toks = _TOKEN.findall(src)
    pos = [0]

    def peek():
        return toks[pos[0]] if pos[0] < len(toks) else None

    def take():
        pos[0] += 1
        return toks[pos[0] - 1]

    def value():
        t = peek()
        if t is None:
            raise Refused("end")
        if t == "(":
            take()
            f = add()
            if take() != ")":
                raise Refused(")")
            return f
        if re.match(r"\d|\.", t):
            take()
            v = float(t)
            return lambda now, et: v
        if re.match(r"[A-Za-z_]", t):
            take()
            if peek() == "(":
                if t != "exp":
                    raise Refused(t)
                take()
                a = add()
                if take() != ")":
                    raise Refused(")")
                return lambda now, et: go_exp(a(now, et))
            if t == "currentTime":
                return lambda now, et: now
            if t == "eventTime":
                return lambda now, et: et
            raise Refused(t)
        raise Refused(t)

    def prefix():
        if peek() == "-":
            take()
            f = prefix()
            return lambda now, et: -f(now, et)
        return value()

    def power():
        f = prefix()
        if peek() == "**":
            raise Refused("** (Go's Pow) is outside this restatement")
        return f

    def div(a, b):
        if b == 0.0:
            if a != a or a == 0.0:
                return math.nan
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b

    def mul():
        f = power()
        while peek() in ("*", "/", "%"):
            op = take()
            g = power()
            if op == "*":
                f = (lambda f, g: lambda now, et: f(now, et) * g(now, et))(f, g)
            elif op == "/":
                f = (lambda f, g: lambda now, et: div(f(now, et), g(now, et)))(f, g)
            else:
                raise Refused("% is outside this restatement")
        return f

    def add():
        f = mul()
        while peek() in ("+", "-"):
            op = take()
            g = mul()
            if op == "+":
                f = (lambda f, g: lambda now, et: f(now, et) + g(now, et))(f, g)
            else:
                f = (lambda f, g: lambda now, et: f(now, et) - g(now, et))(f, g)
        return f

    f = add()
    if peek() is not None:
        raise Refused(peek())
    return f


class Conf:
    """a UserTriggerDaoConf as pg_rtu2i_compile reads it"""

    def __init__(self, weight_expression, event_names=(), event_weight="", event_play_time="", weight_mode="", trigger_count=0, limit=0):
        self.f = compile_expression(weight_expression)
        w, t = parse_pairs(event_weight), parse_pairs(event_play_time)
        if event_weight and not w:
            raise ValueError("EventWeight is empty")
        self.names = list(event_names)
        self.weight = [w.get(n) for n in self.names]
        self.threshold = [t.get(n) for n in self.names]
        self.max_mode = weight_mode == "max"
        self.T = trigger_count if trigger_count else limit
        if not 1 <= self.T <= MAX_TRIGGERS:
            raise ValueError("trigger count")


# ---- the trigger stage -----------------------------------------------------------------------------------------------------------------
def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def request_triggers(conf, table_rows, rows, codes, play_time, times, now):
    """one request → [(row, weight)] in the answer's order, cut to T"""
    weight, first, order = {}, {}, []
    for i in range(len(rows)):
        row, code = int(rows[i]), int(codes[i])
        if row >= table_rows:
            continue
        w = 1.0
        if code < len(conf.names):
            t = conf.threshold[code]
            pt = float(play_time[i]) if play_time is not None else 0.0
            if t is not None and pt <= t:
                continue
            if conf.weight[code] is not None:
                w = conf.weight[code]
        x = w * conf.f(float(int(now)), float(int(times[i])))
        if row in weight:
            if conf.max_mode:
                if x > weight[row]:
                    weight[row] = x
            else:
                weight[row] = weight[row] + x
        else:
            weight[row] = x
            first[row] = i
            order.append(row)
    items = [(r, weight[r]) for r in order if math.isfinite(weight[r])]
    items.sort(key=lambda rw: (-rw[1], first[rw[0]]))                   # (-0.0 == 0.0: it ranks as 0.0)
    return items[:conf.T]


def triggers(conf, table_rows, rows, codes, play_time, times, now):
    """→ (rows [nq][T] uint32, weights [nq][T] float64, counts [nq] uint32)"""
    nq = len(rows)
    out_rows = np.full((nq, conf.T), U32MAX, dtype=np.uint32)
    out_w = np.full((nq, conf.T), -np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        ans = request_triggers(conf, table_rows, rows[q], codes[q], play_time[q] if play_time is not None else None, times[q], now[q])
        for j, (r, w) in enumerate(ans):
            out_rows[q, j] = r
            out_w[q, j] = w
        counts[q] = len(ans)
    return out_rows, out_w, counts


# ---- the expansion ---------------------------------------------------------------------------------------------------------------------
def accumulate_max(sl, trig, prefer):
    """item -> score after the request's triggers: the first term, replaced only by a larger one"""
    score = {}
    for r, p in zip(trig, prefer):
        r, p = int(r), float(p)
        if r >= sl.rows or r not in sl.lists:
            continue
        nb, sm = sl.lists[r]
        for item, s in zip(nb, sm):
            term = s * p
            if item in score:
                if term > score[item]:
                    score[item] = term
            else:
                score[item] = term
    return score


def expand(sl, trig, prefer, k, lists=None):
    """trig[q], prefer[q] → (rows [nq][k] uint64 global ids, scores [nq][k] float64, counts [nq] uint32)"""
    nq = len(trig)
    rows = np.full((nq, k), U64MAX, dtype=np.uint64)
    scores = np.full((nq, k), -np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        ans = sorted(accumulate_max(sl, trig[q], prefer[q]).items(), key=lambda kv: (-kv[1], kv[0]))
        if lists is not None:
            seen = set(int(x) for x in lists[q])
            ans = [(i, s) for i, s in ans if sl.row_offset + i not in seen]
        ans = ans[:k]
        for j, (i, s) in enumerate(ans):
            rows[q, j] = sl.row_offset + i
            scores[q, j] = s
        counts[q] = len(ans)
    return rows, scores, counts


def recall(conf, sl, rows, codes, play_time, times, now, k, lists=None):
    """the recall = the trigger stage, then the expansion of each request's kept triggers"""
    tr, tw, tc = triggers(conf, sl.rows, rows, codes, play_time, times, now)
    return expand(sl, [tr[q, :tc[q]] for q in range(len(rows))], [tw[q, :tc[q]] for q in range(len(rows))], k, lists)
