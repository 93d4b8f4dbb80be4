"""CPU restatement of the U2I2X2I recall's specification (include/pairec_gpu.h, "U2I2X2I recall"): sequential loops
with Python floats, literally.  No GPU, no library.

    hop 1   for every trigger j of the request, in the order given (a row of UINT32_MAX or >= rows contributes nothing):
                for every x of the trigger's X list, in stored order:
                    xPrefer[x] = prefer_j if x is new else xPrefer[x] + prefer_j        # new X stand in order of first appearance
            more than 1024 distinct X: the request is reported (limit "x") and answers 0
            an X whose xPrefer is not finite is dropped
            the kept X's lists hold more than 65536 entries in all: the request is reported (limit "pairs") and answers 0
    hop 2   for every kept X in order of first appearance, for every (item, score) of its list in stored order:
                an item that is one of the request's trigger rows is skipped
                term = xPrefer[x] * float(np.float32 score)                             # an exact widening, then one rounding
                sum rule: score[item] = term if the item is new else score[item] + term
                max rule: score[item] = term if the item is new or term > score[item]
    sum rule: m = the largest score, found with > from 0;  normalize and m > 0:  score = score / m
    order: score descending (-0.0 as 0.0), then row ascending;  with a list: its ids dropped;  the first k;  padding UINT64_MAX / -inf
"""
import math
import struct

import numpy as np

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
U32MAX = 0xFFFFFFFF
MAX_X, MAX_PAIRS, MAX_X_PER_ITEM, MAX_LIST = 1024, 65536, 64, 1024


class XLists:
    """the X table on the host: item -> [x], x -> ([item], [score widened from float32]); keys never uploaded have empty lists"""

    def __init__(self, rows, n_x, row_offset=0):
        self.rows, self.n_x, self.row_offset = int(rows), int(n_x), int(row_offset)
        self.i2x = {}
        self.x2i = {}

    def upload_item2x(self, offsets, x_ids, row0=0):
        x_ids = np.asarray(x_ids, dtype=np.uint32)
        for i in range(len(offsets) - 1):
            self.i2x[row0 + i] = x_ids[int(offsets[i]):int(offsets[i + 1])].tolist()

    def upload_x2item(self, offsets, item_rows, scores, x0=0):
        item_rows = np.asarray(item_rows, dtype=np.uint32)
        scores = np.asarray(scores, dtype=np.float32)
        for i in range(len(offsets) - 1):
            b, e = int(offsets[i]), int(offsets[i + 1])
            self.x2i[x0 + i] = (item_rows[b:e].tolist(), [float(s) for s in scores[b:e]])

    def csr(self):
        """the whole table as the five arrays pg_x2i_recall_host takes"""
        io = np.zeros(self.rows + 1, np.uint64)
        for r, l in self.i2x.items():
            io[r + 1] = len(l)
        io = np.cumsum(io, dtype=np.uint64)
        ii = np.zeros(int(io[-1]), np.uint32)
        for r, l in self.i2x.items():
            ii[int(io[r]):int(io[r + 1])] = l
        xo = np.zeros(self.n_x + 1, np.uint64)
        for x, l in self.x2i.items():
            xo[x + 1] = len(l[0])
        xo = np.cumsum(xo, dtype=np.uint64)
        xr = np.zeros(int(xo[-1]), np.uint32)
        xs = np.zeros(int(xo[-1]), np.float32)
        for x, l in self.x2i.items():
            xr[int(xo[x]):int(xo[x + 1])] = l[0]
            xs[int(xo[x]):int(xo[x + 1])] = l[1]
        return io, ii, xo, xr, xs


def hop1(xl, triggers, prefer):
    """[(x, xPrefer)] in order of first appearance, before anything is dropped"""
    order, pref = [], {}
    for r, p in zip(triggers, prefer):
        r, p = int(r), float(p)
        if r >= xl.rows:
            continue
        for x in xl.i2x.get(r, ()):
            if x in pref:
                pref[x] = pref[x] + p
            else:
                pref[x] = p
                order.append(x)
    return [(x, pref[x]) for x in order]


def limit(xl, triggers, prefer):
    """None, or the limit one request breaks: "x" or "pairs" """
    xs = hop1(xl, triggers, prefer)
    if len(xs) > MAX_X:
        return "x"
    if sum(len(xl.x2i.get(x, ((), ()))[0]) for x, p in xs if math.isfinite(p)) > MAX_PAIRS:
        return "pairs"
    return None


def accumulate(xl, triggers, prefer, max_rule=False):
    """item -> score after both hops (a request beyond a limit: nothing)"""
    if limit(xl, triggers, prefer) is not None:
        return {}
    tset = set(int(r) for r in triggers)
    score = {}
    for x, p in hop1(xl, triggers, prefer):
        if not math.isfinite(p):
            continue
        items, scs = xl.x2i.get(x, ((), ()))
        for item, s in zip(items, scs):
            if item in tset:
                continue
            term = p * s
            if item not in score:
                score[item] = term
            elif not max_rule:
                score[item] = score[item] + term
            elif term > score[item]:
                score[item] = term
    return score


def order_key(s):
    """ascending key = descending score, -0.0 as 0.0; total on every bit pattern"""
    b = struct.unpack("<Q", struct.pack("<d", s))[0]
    if b == 0x8000000000000000:
        b = 0
    asc = (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | 0x8000000000000000)
    return ~asc & 0xFFFFFFFFFFFFFFFF


def ordered(score, normalize):
    """[(row, score)] in the answer's order"""
    m = 0.0
    for s in score.values():
        if s > m:
            m = s
    if normalize and m > 0:
        score = {i: s / m for i, s in score.items()}
    return sorted(score.items(), key=lambda kv: (order_key(kv[1]), kv[0]))


def x2i_recall(xl, triggers, prefer, k, normalize=True, max_rule=False, lists=None):
    """triggers[q], prefer[q] → (rows [nq][k] uint64 global ids, scores [nq][k] float64, counts [nq] uint32)"""
    nq = len(triggers)
    rows = np.full((nq, k), U64MAX, dtype=np.uint64)
    scores = np.full((nq, k), -np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        ans = ordered(accumulate(xl, triggers[q], prefer[q], max_rule), normalize and not max_rule)
        if lists is not None:
            seen = set(int(x) for x in lists[q])
            ans = [(i, s) for i, s in ans if xl.row_offset + i not in seen]      # dropping, then cutting
        ans = ans[:k]
        for j, (i, s) in enumerate(ans):
            rows[q, j] = xl.row_offset + i
            scores[q, j] = s
        counts[q] = len(ans)
    return rows, scores, counts
