"""PriorityAdjustCountFilterV2's specification on the CPU: filter/priority_adjust_count_filter_v2.go:39-103, once
as one statement on arrays (trim2: the definition in include/pairec_gpu.h) and once as an item-by-item transcription of the Go loop
on objects (go_v2), with a stable sort in place of the reference's shuffle + unstable sort and an insertion-ordered map in place of
Go's.  Every order is pg_sort_scores_dev's: key descending with -0.0 equal to +0.0, NaN last, ties by input position (Python's
sorted is stable).  Nothing meets arithmetic: every array is gathered through one list of picks and compared by bits."""
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


def in_score_order(positions, key):
    """`positions` in the order the device's score sort gives them; key: position → float"""
    def k(i):
        s = float(key(i))
        return (1, 0.0) if math.isnan(s) else (0, -s)            # (-(-0.0) == -(+0.0) compares equal: ±0 tie by position)
    return sorted(positions, key=k)


def picks(rules, score, source, mask, planes_f64, real):
    """one request → [(position, rule index, key came from the plane)] in output order"""
    dup = set() if mask is None else {e for e in real if bin(int(mask[e])).count("1") > 1}
    taken, out, acc = set(), [], 0
    for c, (s_c, typ, cnt) in enumerate(rules):
        key = {}
        for e in real:
            if e in dup:
                if (int(mask[e]) >> s_c) & 1:
                    key[e] = (planes_f64[s_c][e], True)
            elif source is None or int(source[e]) == s_c:
                key[e] = (score[e], False)
        order = in_score_order([e for e in real if e in key], lambda e: key[e][0])
        limit = cnt if typ == FIX else max(0, cnt - acc)
        mine = [e for e in order if e not in taken][:limit]
        taken.update(mine)
        out += [(e, c, key[e][1]) for e in mine]
        if typ != FIX:
            acc += len(mine)
    return out


def trim2(rules, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """rules = [(source, FIX | ACCUMULATE, count)] → (rows, score, source, planes_f64, source_mask, planes_f32, count) as
    Context.candidates_trim2 returns them"""
    rows = np.asarray(rows, np.uint64)
    score = np.asarray(score, np.float64)
    nq, cap = rows.shape
    oc = out_cap(rules, cap)
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
        real = [i for i in range(n_valid) if int(rows[q, i]) != U64MAX]
        keep = picks(rules, score[q], None if source is None else source[q], None if source_mask is None else source_mask[q],
                     None if p64 is None else p64[:, q], real)
        n = len(keep)
        assert n <= oc
        o_count[q] = n
        if n == 0:
            continue
        at = np.array([e for e, _, _ in keep], np.int64)
        via = np.array([rules[c][0] for _, c, _ in keep], np.int64)
        o_rows[q, :n] = rows[q, at]
        o_score[q, :n] = sbits[q, at]
        plane = np.flatnonzero(np.array([p for _, _, p in keep], bool))
        if plane.size:
            o_score[q, plane] = p64.view(np.uint64)[via[plane], q, at[plane]]
        if o_source is not None:
            o_source[q, :n] = via
        if o_p64 is not None:
            o_p64[:, q, :n] = p64.view(np.uint64)[:, q, at]
        if o_mask is not None:
            o_mask[q, :n] = np.asarray(source_mask, np.uint32)[q, at]
        if o_p32 is not None:
            o_p32[:, q, :n] = p32.view(np.uint32)[:, q, at]
    return (o_rows, o_score.view(np.float64), o_source, None if o_p64 is None else o_p64.view(np.float64), o_mask,
            None if o_p32 is None else o_p32.view(np.float32), o_count)


# ---- the reference's loop, item by item ------------------------------------------------------------------------------------------

class Item:
    def __init__(self, id_, score, retrieve_id, recall_scores=None):
        self.Id, self.Score, self.RetrieveId, self.RecallScores = id_, score, retrieve_id, dict(recall_scores or {})


def unique_filter(items):
    """UniqueFilter.doFilter (filter/unique_filter.go:27-52): the first item of an id stays; a repeat leaves its recall's score in
    RecallScores (the first item's own score goes in when the first repeat arrives, and a repeat of a recall overwrites it)"""
    seen, out = {}, []
    for it in items:
        first = seen.get(it.Id)
        if first is None:
            seen[it.Id] = it
            out.append(it)
        else:
            if not first.RecallScores:
                first.RecallScores[first.RetrieveId] = first.Score
            first.RecallScores[it.RetrieveId] = it.Score
    return out


def go_v2(configs, items):
    """PriorityAdjustCountFilterV2.doFilter (:39-103).  configs = [{"RecallName", "Type": "fix" | "accumulator", "Count"}]; the
    items are changed as the reference changes them (RetrieveId, Score) and the kept ones returned in order."""
    new_items = []
    recall_to_item_map = {}
    duplicate_recall_item_map = {}                                  # (a dict keeps insertion order: input order among equal keys)
    accumulator = 0

    def sort_items(lst):                                           # :47-52 without the shuffle, stable
        lst[:] = in_score_order(lst, lambda it: it.Score)

    for item in items:                                             # :54-60
        if len(item.RecallScores) > 1:
            duplicate_recall_item_map[id(item)] = item
        else:
            recall_to_item_map.setdefault(item.RetrieveId, []).append(item)
    for config in configs:                                         # :62-98
        recall_items = list(recall_to_item_map.get(config["RecallName"], []))
        for item in duplicate_recall_item_map.values():            # :66-72
            if config["RecallName"] in item.RecallScores:
                item.RetrieveId = config["RecallName"]
                item.Score = item.RecallScores[config["RecallName"]]
                recall_items.append(item)
        sort_items(recall_items)
        if config["Type"] == "fix":                                # :76-84
            i = 0
            while i < len(recall_items) and i < config["Count"]:
                new_items.append(recall_items[i])
                duplicate_recall_item_map.pop(id(recall_items[i]), None)
                i += 1
        elif config["Type"] == "accumulator":                      # :85-97
            count = config["Count"] - accumulator
            i = 0
            while i < len(recall_items) and i < count:
                new_items.append(recall_items[i])
                duplicate_recall_item_map.pop(id(recall_items[i]), None)
                accumulator += 1
                i += 1
    return new_items


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
