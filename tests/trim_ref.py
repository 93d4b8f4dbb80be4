"""The candidate trim's specification on the CPU: filter/priority_adjust_count_filter.go:92-203 with
ensureDiversity == false, and filter/adjust_count_filter.go:58-71 with ShuffleItem false, restated on arrays.  The order is
pg_sort_scores_dev's: score descending with -0.0 equal to +0.0, NaN last, ties by input position (Python's sorted is stable).
Nothing meets arithmetic: every array is gathered through one permutation and compared by bits."""
import math

import numpy as np

U64MAX = 0xFFFFFFFFFFFFFFFF
NAN_BITS = 0x7FF8000000000000
NEG_INF_BITS = 0xFFF0000000000000
FIX, ACCUMULATE, ANY = 0, 1, 0xFF
MAX_RULES, MAX_SOURCES, MAX_PLANES, MAX_CAP, CHUNK = 8, 8, 8, 16384, 1024


def out_cap(rules, cap):
    """no request can keep more: the FIX counts and the largest ACCUMULATE count"""
    fix = sum(c for _, t, c in rules if t == FIX)
    acc = max([c for _, t, c in rules if t == ACCUMULATE], default=0)
    return min(cap, fix + acc)


def score_order(score, real):
    """the positions in `real`, in the order the device's score sort gives them"""
    def key(i):
        s = float(score[i])
        return (1, 0.0) if math.isnan(s) else (0, -s)            # (-(-0.0) == -(+0.0) compares equal: ±0 tie by position)
    return sorted(real, key=key)


def picks(rules, score, source, real):
    """one request: the input positions kept, in output order"""
    order = score_order(score, real)
    if len(rules) == 1 and rules[0][0] == ANY:
        # adjust_count_filter.go:58-71: the first RetainNum of the sorted list (one FIX quota over every source; an ACCUMULATE
        # one starts from an empty accumulator and is the same)
        return order[:rules[0][2]]
    by_source = {}
    for i in order:                                                # :103-104
        by_source.setdefault(int(source[i]), []).append(i)
    out, acc = [], 0
    for src, typ, cnt in rules:                                    # :143-203
        lst = by_source.get(src, [])
        if typ == FIX:
            out += lst[:cnt]                                       # :146-150 (the accumulator stays)
        else:
            n = cnt - acc                                          # :193
            assert n >= 0
            take = lst[:n]                                         # :194-200
            out += take
            acc += len(take)
    return out


def trim(rules, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """→ (rows, score, source, planes_f64, source_mask, planes_f32, count) as Context.candidates_trim returns them"""
    rows = np.asarray(rows, np.uint64)
    score = np.asarray(score, np.float64)
    nq, cap = rows.shape
    oc = out_cap(rules, cap)
    o_rows = np.full((nq, oc), U64MAX, np.uint64)
    o_score = np.full((nq, oc), NEG_INF_BITS, np.uint64)
    o_source = None if source is None else np.full((nq, oc), 0xFF, np.uint8)
    o_p64 = None if planes_f64 is None else np.full((len(planes_f64), nq, oc), NAN_BITS, np.uint64)
    o_mask = None if source_mask is None else np.zeros((nq, oc), np.uint32)
    o_p32 = None if planes_f32 is None else np.zeros((len(planes_f32), nq, oc), np.uint32)
    o_count = np.zeros(nq, np.uint32)
    sbits = score.view(np.uint64)
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        real = [i for i in range(n_valid) if int(rows[q, i]) != U64MAX]
        keep = np.array(picks(rules, score[q], None if source is None else source[q], real), np.int64)
        n = keep.size
        assert n <= oc
        o_count[q] = n
        o_rows[q, :n] = rows[q, keep]
        o_score[q, :n] = sbits[q, keep]
        if o_source is not None:
            o_source[q, :n] = np.asarray(source, np.uint8)[q, keep]
        if o_p64 is not None:
            o_p64[:, q, :n] = np.asarray(planes_f64, np.float64).view(np.uint64)[:, q, keep]
        if o_mask is not None:
            o_mask[q, :n] = np.asarray(source_mask, np.uint32)[q, keep]
        if o_p32 is not None:
            o_p32[:, q, :n] = np.asarray(planes_f32, np.float32).view(np.uint32)[:, q, keep]
    return (o_rows, o_score.view(np.float64), o_source, None if o_p64 is None else o_p64.view(np.float64), o_mask,
            None if o_p32 is None else o_p32.view(np.float32), o_count)


def same(got, want):
    """every output array by bits; an array absent on one side is absent on the other"""
    names = ("rows", "score", "source", "planes_f64", "source_mask", "planes_f32", "count")
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert (g is None) == (w is None), name
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        elif g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), "%s differs at %s" % (name, np.argwhere(g != w)[:4].tolist())
