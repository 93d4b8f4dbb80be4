"""The candidate blend's specification on the CPU: filter/snake_filter.go:173-241 and
filter/completely_fair_count_filter.go:34-94 restated on arrays.  Every order is pg_sort_scores_dev's: key descending with -0.0
equal to +0.0, NaN last, ties by input position (Python's sorted is stable).  Nothing meets arithmetic: every array is gathered
through one list of picks and compared by bits."""
import math

import numpy as np

U64MAX = 0xFFFFFFFFFFFFFFFF
NAN_BITS = 0x7FF8000000000000
NEG_INF_BITS = 0xFFF0000000000000
SNAKE_REFILL, SNAKE_SKIP, FAIR = 0, 1, 2
MAX_SOURCES, MAX_PLANES, MAX_CAP, LDS_LIST = 8, 8, 16384, 2064


def out_cap(conf, cap):
    return min(cap, conf[1])


def in_score_order(positions, key):
    """`positions` in the order the device's score sort gives them; key: position → float"""
    def k(i):
        s = float(key(i))
        return (1, 0.0) if math.isnan(s) else (0, -s)            # (-(-0.0) == -(+0.0) compares equal: ±0 tie by position)
    return sorted(positions, key=k)


def snake_lists(entries, score, source, mask, planes_f64, real):
    """one request: per config entry [(position, key)] in score order of the key (snake_filter.go:63-67,188-200)"""
    lists = []
    several = {} if mask is None else {e: int(mask[e]) for e in real if bin(int(mask[e])).count("1") > 1}
    for s_i, _ in entries:
        key = {}
        for e in real:
            if source[e] == s_i:
                key[e] = score[e]
            elif (several.get(e, 0) >> s_i) & 1:
                key[e] = planes_f64[s_i][e]
        order = in_score_order([e for e in real if e in key], key.__getitem__)
        lists.append([(e, key[e]) for e in order])
    return lists


def snake_picks(conf, score, source, mask, planes_f64, real, rounds=None):
    """one request → [(position, entry index)] in pick order, cut to retain_num; `rounds` collects every round's picks per entry"""
    mode, retain_num, entries = conf
    lists = snake_lists(entries, score, source, mask, planes_f64, real)
    cursor = [0] * len(entries)
    taken, picks, size = set(), [], 0
    while size < retain_num:                                       # :212-227
        got = 0
        this_round = []
        for i, (_, weight) in enumerate(entries):
            slots, mine = 0, []
            while slots < weight and cursor[i] < len(lists[i]):    # Next, :76-109
                e = lists[i][cursor[i]][0]
                cursor[i] += 1
                if e not in taken:
                    taken.add(e)
                    mine.append(e)
                    slots += 1
                elif mode == SNAKE_SKIP:
                    slots += 1
            picks += [(e, i) for e in mine]
            got += len(mine)
            this_round.append(mine)
        if rounds is not None:
            rounds.append(this_round)
        if got == 0:
            break
        size += got
    return picks[:retain_num]                                      # :229-231


def fair_picks(retain_num, score, source, real):
    """one request → the positions kept, in output order"""
    retain = min(retain_num, len(real))
    order = in_score_order(real, lambda e: score[e])
    by_source, names = {}, []
    for e in order:                                                # :59-65
        s = int(source[e])
        if s not in by_source:
            by_source[s] = []
            names.append(s)
        by_source[s].append(e)
    out, count = [], 0
    while count < retain:                                          # :72-89
        i = count % len(names)
        lst = by_source[names[i]]
        out.append(lst.pop(0))
        count += 1
        if not lst:
            names[i] = names[-1]
            names.pop()
    return out


def blend(conf, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """conf = (mode, retain_num, [(source, weight)]) → (rows, score, source, planes_f64, source_mask, planes_f32, count) as
    Context.candidates_blend returns them"""
    mode, retain_num, entries = conf
    rows = np.asarray(rows, np.uint64)
    score = np.asarray(score, np.float64)
    nq, cap = rows.shape
    oc = out_cap(conf, cap)
    p64 = None if planes_f64 is None else np.asarray(planes_f64, np.float64)
    p32 = None if planes_f32 is None else np.asarray(planes_f32, np.float32)
    o_rows = np.full((nq, oc), U64MAX, np.uint64)
    o_score = np.full((nq, oc), NEG_INF_BITS, np.uint64)
    o_source = None if source is None else np.full((nq, oc), 0xFF, np.uint8)
    o_p64 = None if p64 is None else np.full((len(p64), nq, oc), NAN_BITS, np.uint64)
    o_mask = None if source_mask is None else np.zeros((nq, oc), np.uint32)
    o_p32 = None if p32 is None else np.zeros((len(p32), nq, oc), np.uint32)
    o_count = np.zeros(nq, np.uint32)
    sbits = score.view(np.uint64)
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        if source is not None:
            src = [int(s) for s in source[q]]
        else:                                                      # one source: the snake's single entry names it
            src = [0 if mode == FAIR else entries[0][0]] * cap
        real = [i for i in range(n_valid) if int(rows[q, i]) != U64MAX and src[i] < MAX_SOURCES]
        if mode == FAIR:
            keep = [(e, None) for e in fair_picks(retain_num, score[q], src, real)]
        else:
            keep = snake_picks(conf, score[q], src, None if source_mask is None else source_mask[q],
                               None if p64 is None else p64[:, q], real)
        n = len(keep)
        assert n <= oc
        o_count[q] = n
        if n == 0:
            continue
        at = np.array([e for e, _ in keep], np.int64)
        o_rows[q, :n] = rows[q, at]
        o_score[q, :n] = sbits[q, at]
        if mode != FAIR:                                           # :83-88: the picking list's name, and its score
            via = np.array([entries[i][0] for _, i in keep], np.int64)
            other = np.flatnonzero(np.array(src, np.int64)[at] != via)
            if other.size:
                o_score[q, other] = p64.view(np.uint64)[via[other], q, at[other]]
        if o_source is not None:
            o_source[q, :n] = np.asarray(source, np.uint8)[q, at] if mode == FAIR else via
        if o_p64 is not None:
            o_p64[:, q, :n] = p64.view(np.uint64)[:, q, at]
        if o_mask is not None:
            o_mask[q, :n] = np.asarray(source_mask, np.uint32)[q, at]
        if o_p32 is not None:
            o_p32[:, q, :n] = p32.view(np.uint32)[:, q, at]
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
