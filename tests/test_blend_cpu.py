"""CPU checks behind the candidate blend: tests/blend_ref.py — the specification the GPU tests compare with —
against a literal, item-by-item transcription of the reference's loops (filter/snake_filter.go:39-241,
filter/completely_fair_count_filter.go:34-94) with one object per item; the reference's own test cases (tests/golden/
blend_filters.json); pg_candidates_blend_host, the library's host statement, against blend_ref by bits; pg_blend_out_cap and every
refusal; the round property of snake_filter_test.go; and the host mirror's config parse."""
import copy
import ctypes as C
import functools
import json
import math
import os
import re

import numpy as np
import pytest

import blend_ref as ref
import pairec_amd as pa
from pairec_amd import _lib
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFILL, SKIP, FAIR = ref.SNAKE_REFILL, ref.SNAKE_SKIP, ref.FAIR
INVALID, UNSUPPORTED = -1, -4
with open(os.path.join(ROOT, "tests", "golden", "blend_filters.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
MODES = {"SNAKE_REFILL": REFILL, "SNAKE_SKIP": SKIP, "FAIR": FAIR}


# ---- the reference's loops, item by item --------------------------------------------------------------------------------------------

class Item:
    def __init__(self, pos, score, retrieve_id, recall_scores):
        self.Id, self.Score, self.RetrieveId, self.RecallScores = pos, score, retrieve_id, recall_scores


def go_sorted_desc(items, score_of):
    """sort.Slice(items, score(i) > score(j)) / sort.Sort(sort.Reverse(ItemScoreSlice)) with the order among equal keys fixed:
    entries neither of which is greater keep their input order, and a NaN (greater than nothing) goes behind every number"""
    def cmp(a, b):
        x, y = score_of(a), score_of(b)
        if math.isnan(x) or math.isnan(y):
            return (1 if math.isnan(x) else 0) - (1 if math.isnan(y) else 0)
        return -1 if x > y else (1 if y > x else 0)
    return sorted(items, key=functools.cmp_to_key(cmp))


class SnakeItemIterator:
    def __init__(self, config, already, skip):
        self.items, self.scoreMap, self.index = [], {}, 0
        self.recallName, self.weight, self.skip, self.already = config["RecallName"], config["Weight"], skip, already

    def AddItem(self, item):                                       # :61-68
        self.items.append(item)
        if item.RetrieveId != self.recallName:
            self.scoreMap[item.Id] = item.RecallScores[self.recallName]
        else:
            self.scoreMap[item.Id] = item.Score

    def Sort(self):                                                # :71-75
        self.items = go_sorted_desc(self.items, lambda it: self.scoreMap[it.Id])

    def Next(self, size):                                          # :76-109
        ret, i = [], 0
        while i < size and self.index < len(self.items):
            item = self.items[self.index]
            if item.Id not in self.already:
                self.already[item.Id] = True
                if item.RetrieveId != self.recallName:
                    item.RetrieveId = self.recallName
                    if self.recallName in item.RecallScores:
                        item.Score = item.RecallScores[self.recallName]
                self.index += 1
                i += 1
                ret.append(item)
            else:
                self.index += 1
                if self.skip:
                    i += 1
        return ret


def go_snake(configs, retain_num, skip, items):
    """SnakeFilter.doFilter (:173-241) without the debug property"""
    new_items, already = [], {}
    iterators = [SnakeItemIterator(c, already, skip) for c in configs]
    by_name = {c["RecallName"]: it for c, it in zip(configs, iterators)}
    for item in items:                                             # :187-206
        if len(item.RecallScores) > 1:
            if item.RetrieveId in by_name:
                by_name[item.RetrieveId].AddItem(item)
            for recall_name in item.RecallScores:
                if recall_name == item.RetrieveId:
                    continue
                if recall_name in by_name:
                    by_name[recall_name].AddItem(item)
        elif item.RetrieveId in by_name:
            by_name[item.RetrieveId].AddItem(item)
    for it in by_name.values():
        it.Sort()
    size = 0
    while size < retain_num:                                       # :212-227
        iter_size = 0
        for i, config in enumerate(configs):
            got = iterators[i].Next(config["Weight"])
            if got:
                iter_size += len(got)
                new_items += got
        if iter_size == 0:
            break
        size += iter_size
    return new_items[:retain_num] if len(new_items) > retain_num else new_items


def go_fair(retain_num, items):
    """CompletelyFairCountFilter.doFilter (:34-94)"""
    if len(items) == 0:
        return []
    if len(items) <= retain_num:
        retain_num = len(items)
    new_items, recall_to_item_map, recall_names = [], {}, []
    items = go_sorted_desc(items, lambda it: it.Score)
    for item in items:
        recall_to_item_map.setdefault(item.RetrieveId, []).append(item)
        if item.RetrieveId not in recall_names:
            recall_names.append(item.RetrieveId)
    count, recall_names_count = 0, len(recall_names)
    while count < retain_num:
        i = count % recall_names_count
        item_list = recall_to_item_map[recall_names[i]]
        new_items.append(item_list[0])
        count += 1
        if len(item_list) == 1:
            recall_names[i] = recall_names[recall_names_count - 1]
            recall_names = recall_names[:recall_names_count - 1]
            recall_names_count -= 1
        else:
            recall_to_item_map[recall_names[i]] = item_list[1:]
    return new_items


def literal(conf, rows, score, source, count, p64, mask, p32):
    """the transcription over the same arrays: items are built as the fan-in's outputs describe them (RetrieveId = the source,
    RecallScores = the planes the mask names), the filters run on objects, and what they return is written out"""
    mode, retain_num, entries = conf
    nq, cap = rows.shape
    oc = ref.out_cap(conf, cap)
    o_rows = np.full((nq, oc), ref.U64MAX, np.uint64)
    o_score = np.full((nq, oc), ref.NEG_INF_BITS, np.uint64).view(np.float64)
    o_source = np.full((nq, oc), 0xFF, np.uint8)
    o_p64 = np.full((len(p64), nq, oc), ref.NAN_BITS, np.uint64).view(np.float64)
    o_mask = None if mask is None else np.zeros((nq, oc), np.uint32)
    o_p32 = np.zeros((len(p32), nq, oc), np.float32)
    o_count = np.zeros(nq, np.uint32)
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        items = []
        for i in range(n_valid):
            if int(rows[q, i]) == ref.U64MAX or source[q, i] >= ref.MAX_SOURCES:
                continue
            scores = {}
            if mask is not None:
                scores = {"s%d" % b: (p64[b, q, i] if b < len(p64) else 0.0) for b in range(32) if (int(mask[q, i]) >> b) & 1}
            items.append(Item(i, score[q, i], "s%d" % source[q, i], scores))
        if mode == FAIR:
            kept = go_fair(retain_num, items)
        else:
            kept = go_snake([{"RecallName": "s%d" % s, "Weight": w} for s, w in entries], retain_num, mode == SKIP, items)
        o_count[q] = len(kept)
        for slot, it in enumerate(kept):
            i = it.Id
            o_rows[q, slot], o_score[q, slot], o_source[q, slot] = rows[q, i], it.Score, int(it.RetrieveId[1:])
            if mask is not None:
                o_mask[q, slot] = mask[q, i]
            o_p64[:, q, slot] = p64[:, q, i]
            o_p32[:, q, slot] = p32[:, q, i]
    return o_rows, o_score, o_source, o_p64, o_mask, o_p32, o_count


# ---- random merges --------------------------------------------------------------------------------------------------------------------

NAN_PAYLOAD = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
VALUES = np.array([-np.inf, -2.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.0, np.inf, NAN_PAYLOAD, 5e-324, -5e-324])


def merged(rng, nq, cap, n_src, with_count=True, overlap=0.4, values=VALUES):
    """what a fan-in could have left: few distinct scores (±0.0, infinities, NaN and subnormals among them), padding sprinkled
    in the middle, sources past the limit, masks that name the first source and some others, every carried array distinct"""
    rows = rng.permutation(nq * cap).reshape(nq, cap).astype(np.uint64) + np.uint64(1 << 33)
    rows[rng.random((nq, cap)) < 0.08] = ref.U64MAX
    score = values[rng.integers(0, values.size, (nq, cap))]
    source = rng.integers(0, n_src, (nq, cap)).astype(np.uint8)
    source[rng.random((nq, cap)) < 0.03] = 9                        # (a source past the limit is padding)
    count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32) if with_count else None
    p64 = values[rng.integers(0, values.size, (n_src, nq, cap))]
    others = np.zeros((nq, cap), np.uint32)
    for b in range(n_src):
        others |= (rng.random((nq, cap)) < overlap).astype(np.uint32) << np.uint32(b)
    mask = (others | (np.uint32(1) << (source.astype(np.uint32) & 31))).astype(np.uint32)
    p32 = rng.standard_normal((2, nq, cap)).astype(np.float32)
    return rows, score, source, count, p64, mask, p32


def random_conf(rng, n_src, cap):
    mode = int(rng.integers(0, 3))
    retain = int(rng.choice([1, 3, cap // 3, cap // 2, cap, cap + 7]))
    named = rng.permutation(n_src)[:int(rng.integers(1, n_src + 1))]
    entries = [(int(s), int(rng.integers(0, 6))) for s in named]
    if all(w == 0 for _, w in entries):
        entries[0] = (entries[0][0], 2)
    return (mode, max(retain, 1), entries)


def random_cases(n, seed):
    rng = np.random.default_rng(seed)
    for k in range(n):
        n_src = int(rng.integers(1, 6))
        cap = int(rng.integers(1, 70))
        data = merged(rng, 2, cap, n_src, with_count=bool(k % 2), overlap=float(rng.choice([0.0, 0.3, 1.0])))
        yield random_conf(rng, n_src, cap), data


def test_blend_ref_reads_the_filters_as_their_loops_do():
    n = {REFILL: 0, SKIP: 0, FAIR: 0}
    for conf, (rows, score, source, count, p64, mask, p32) in random_cases(300, 41):
        ref.same(ref.blend(conf, rows, score, source, count, p64, mask, p32), literal(conf, rows, score, source, count, p64, mask, p32))
        n[conf[0]] += 1
    assert min(n.values()) > 50
    # without a mask nothing is reached through a second recall
    for conf, (rows, score, source, count, p64, _, p32) in random_cases(40, 42):
        ref.same(ref.blend(conf, rows, score, source, count, p64, None, p32), literal(conf, rows, score, source, count, p64, None, p32))


def test_host_statement_equals_blend_ref_by_bits():
    for conf, (rows, score, source, count, p64, mask, p32) in random_cases(300, 41):
        ref.same(pa.candidates_blend_host(conf, rows, score, source, count, p64, mask, p32),
                 ref.blend(conf, rows, score, source, count, p64, mask, p32))
    for conf, (rows, score, source, count, p64, mask, p32) in random_cases(60, 43):
        for kw in ({}, {"source": source}, {"count": count}, {"planes_f64": p64}, {"planes_f32": p32},
                   {"source": source, "planes_f64": p64, "source_mask": mask}):
            c = conf
            if "source" not in kw and conf[0] != FAIR:                  # (a snake without sources names one)
                c = (conf[0], conf[1], [(conf[2][0][0], max(conf[2][0][1], 1))])
            ref.same(pa.candidates_blend_host(c, rows, score, **kw), ref.blend(c, rows, score, **kw))


def test_ties_nan_and_the_rewrite():
    # two recalls; item 12 stands in both lists: first in recall 0 (score 1.0), recall 1 scores it 9.0
    rows = np.arange(10, 16, dtype=np.uint64).reshape(1, -1)
    score = np.array([[2.0, NAN_PAYLOAD, 1.0, -0.0, 0.0, 5.0]])
    source = np.array([[0, 0, 0, 1, 1, 1]], np.uint8)
    mask = np.array([[1, 1, 3, 2, 2, 2]], np.uint32)
    p64 = np.full((2, 1, 6), np.nan)
    p64[0, 0, :3], p64[1, 0, 3:], p64[1, 0, 2] = score[0, :3], score[0, 3:], 9.0
    got = ref.blend((REFILL, 6, [(0, 1), (1, 1)]), rows, score, source, None, p64, mask)
    # lists: recall 0 = 10 (2.0), 12 (1.0), 11 (NaN); recall 1 = 12 (9.0), 15 (5.0), 13 (-0.0), 14 (0.0): ±0 tie by position
    assert got[0][0].tolist() == [10, 12, 11, 15, 13, 14] and got[2][0].tolist() == [0, 1, 0, 1, 1, 1] and got[6][0] == 6
    assert got[1][0, 1] == 9.0 and got[1].view(np.uint64)[0, 2] == 0x7FF8000000000123 and got[1].view(np.uint64)[0, 4] == 1 << 63
    skip = ref.blend((SKIP, 6, [(0, 1), (1, 1)]), rows, score, source, None, p64, mask)
    # SKIP: round 2 spends recall 0's slot on 12, taken already
    assert skip[0][0].tolist() == [10, 12, 15, 11, 13, 14]
    # an item whose first source no entry names, reached through the recall its mask names
    got = ref.blend((REFILL, 6, [(1, 2)]), rows, score, source, None, p64, mask)
    assert got[0][0].tolist()[:4] == [12, 15, 13, 14] and got[6][0] == 4 and got[2][0].tolist() == [1, 1, 1, 1, 0xFF, 0xFF]
    ref.same(pa.candidates_blend_host((REFILL, 6, [(1, 2)]), rows, score, source, None, p64, mask), got)


def test_skip_round_without_a_pick_ends_the_walk():
    # every item in both recalls, same order: after recall 0 took one, recall 1's slot goes to the same item, and in the end a
    # round picks nothing although recall 1's list is not through
    rows = np.arange(4, dtype=np.uint64).reshape(1, -1)
    score = np.array([[4.0, 3.0, 2.0, 1.0]])
    source = np.zeros((1, 4), np.uint8)
    mask = np.full((1, 4), 3, np.uint32)
    p64 = np.stack([score, score])
    got = ref.blend((SKIP, 4, [(0, 2), (1, 1)]), rows, score, source, None, p64, mask)
    # round 1: recall 0 takes 0, 1; recall 1 looks at 0.  round 2: recall 0 takes 2, 3; recall 1 looks at 1.  round 3: nothing.
    assert got[0][0].tolist() == [0, 1, 2, 3] and got[6][0] == 4
    got = ref.blend((SKIP, 4, [(1, 1), (0, 2)]), rows, score, source, None, p64, mask)
    # round 1: recall 1 takes 0; recall 0 looks at 0, takes 1.  round 2: recall 1 looks at 1; recall 0 takes 2, 3.  size 4: done
    assert got[0][0].tolist() == [0, 1, 2, 3] and got[2][0].tolist() == [1, 0, 0, 0]
    rows = np.arange(6, dtype=np.uint64).reshape(1, -1)
    score = np.array([[6.0, 5.0, 4.0, 3.0, 2.0, 1.0]])
    mask = np.full((1, 6), 3, np.uint32)
    p64 = np.stack([score, score])
    got = ref.blend((SKIP, 6, [(0, 1), (1, 1)]), rows, score, np.zeros((1, 6), np.uint8), None, p64, mask)
    # recall 1 always looks at what recall 0 took the round before: rounds give 0, 1, 2, 3, 4, 5 one at a time
    assert got[6][0] == 6
    one = ref.blend((SKIP, 6, [(0, 1), (1, 1)]), rows, score, np.zeros((1, 6), np.uint8), None, p64, np.where(np.arange(6) < 1, 3, 1).astype(np.uint32).reshape(1, -1))
    assert one[6][0] == 6
    # ... and the quirk: recall 0 is through, recall 1 spends its only slot on a taken item → a round without a pick, fresh entries left
    score = np.array([[6.0, 5.0, 4.0, 3.0]])
    source = np.array([[0, 0, 1, 1]], np.uint8)
    mask = np.array([[3, 3, 2, 2]], np.uint32)
    p64 = np.array([[[6.0, 5.0, np.nan, np.nan]], [[9.0, 8.0, 4.0, 3.0]]])
    got = ref.blend((SKIP, 4, [(0, 2), (1, 1)]), rows[:, :4], score, source, None, p64, mask)
    # round 1: recall 0 takes 0, 1; recall 1 looks at 0 (9.0).  round 2: recall 0 has nothing; recall 1 looks at 1 (8.0): no pick, the end
    assert got[0][0].tolist() == [0, 1, ref.U64MAX, ref.U64MAX] and got[6][0] == 2
    ref.same(pa.candidates_blend_host((SKIP, 4, [(0, 2), (1, 1)]), rows[:, :4], score, source, None, p64, mask), got)
    refill = ref.blend((REFILL, 4, [(0, 2), (1, 1)]), rows[:, :4], score, source, None, p64, mask)
    assert refill[0][0].tolist() == [0, 1, 2, 3]


# ---- the reference's own cases ------------------------------------------------------------------------------------------------------

def golden_arrays(case):
    items = case["items"]
    rows = np.array([[it[0] for it in items]], np.uint64)
    score = np.array([[it[1] for it in items]], np.float64)
    source = np.array([[it[2] for it in items]], np.uint8)
    conf = (MODES[case["mode"]], case["retain_num"], [tuple(e) for e in case["entries"]])
    return conf, rows, score, source


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_the_reference_tests_answers(case):
    conf, rows, score, source = golden_arrays(case)
    n = len(case["expect_ids"])
    for got in (ref.blend(conf, rows, score, source), pa.candidates_blend_host(conf, rows, score, source)):
        assert got[6][0] == n == len(case["expect_sources"])
        assert got[0][0, :n].tolist() == case["expect_ids"]
        assert got[2][0, :n].tolist() == case["expect_sources"]
        assert got[1][0, :n].tolist() == [float(score[0, rows[0].tolist().index(i)]) for i in case["expect_ids"]]
        assert (got[0][0, n:] == ref.U64MAX).all()


def test_golden_fixture_is_data_with_citations():
    assert {c["name"] for c in GOLDEN} >= {"snake_weights_1_1_1", "snake_weights_3_3_4", "snake_recall_absent", "snake_recall_not_configured",
                                           "fair_retain_10", "fair_retain_100_over_20"}
    for c in GOLDEN:
        assert re.match(r"filter/(snake_filter|completely_fair_count_filter)_test\.go:\d+-\d+$", c["cites"]), c["name"]
    assert all("tie" in c["pins"] for c in GOLDEN if c["mode"] == "FAIR")


# ---- the round property (snake_filter_test.go:245-318, :385-460) ----------------------------------------------------------------

def test_refill_rounds_give_every_entry_its_weight_while_no_list_runs_dry():
    rng = np.random.default_rng(7)
    checked = 0
    for _ in range(60):
        n_src, cap = int(rng.integers(2, 6)), 64
        rows, score, source, count, p64, mask, p32 = merged(rng, 1, cap, n_src, with_count=False, overlap=0.5,
                                                            values=np.arange(1.0, 40.0))
        named = rng.permutation(n_src)[:int(rng.integers(1, n_src + 1))]
        entries = [(int(s), int(rng.integers(1, 4))) for s in named]
        retain = int(rng.integers(1, 20))
        conf = (REFILL, retain, entries)
        real = [i for i in range(cap) if int(rows[0, i]) != ref.U64MAX and source[0, i] < ref.MAX_SOURCES]
        rounds = []
        ref.snake_picks(conf, score[0], [int(s) for s in source[0]], mask[0], p64[:, 0], real, rounds)
        got = pa.candidates_blend_host(conf, rows, score, source, count, p64, mask, p32)
        at = 0
        for rnd in rounds:
            if any(len(mine) < w for mine, (_, w) in zip(rnd, entries)):
                break                                                   # a list ran dry: the property holds up to here
            for (s, w) in entries:
                seg = got[2][0, at:min(at + w, int(got[6][0]))]
                assert seg.size == min(w, max(int(got[6][0]) - at, 0)) and (seg == s).all()
                at += w
                checked += seg.size
    assert checked > 300


# ---- pg_blend_out_cap and the refusals ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conf,cap,want", [
    ((REFILL, 5, [(0, 1)]), 100, 5), ((SKIP, 500, [(0, 1), (3, 0)]), 100, 100), ((FAIR, 2000, []), 8000, 2000),
    ((FAIR, 0xFFFFFFFF, [(9, 0)] * 3), 16384, 16384), ((REFILL, 1, [(s, 0xFFFFFFFF) for s in range(8)]), 1, 1),
])
def test_out_cap(conf, cap, want):
    assert pa.blend_out_cap(conf, cap) == want == ref.out_cap(conf, cap)
    assert pa.Context.blend_out_cap(conf, cap) == want


@pytest.mark.parametrize("conf,cap,code,word", [
    ((3, 5, [(0, 1)]), 10, INVALID, "mode 3"),
    ((REFILL, 0, [(0, 1)]), 10, INVALID, "retain_num"),
    ((FAIR, 0, []), 10, INVALID, "retain_num"),
    ((REFILL, 5, []), 10, INVALID, "without entries"),
    ((SKIP, 5, [(8, 1)]), 10, INVALID, "source 8"),
    ((REFILL, 5, [(0, 1), (1, 2), (0, 3)]), 10, INVALID, "twice"),
    ((REFILL, 5, [(0, 0), (1, 0)]), 10, INVALID, "every weight is 0"),
    ((SKIP, 5, [(s % 8, 1) for s in range(9)]), 10, UNSUPPORTED, "n_entries"),
    ((REFILL, 5, [(0, 1)]), 0, UNSUPPORTED, "cap"),
    ((FAIR, 5, []), 16385, UNSUPPORTED, "cap"),
])
def test_refused_confs(conf, cap, code, word):
    with pytest.raises(PgError) as ei:
        pa.blend_out_cap(conf, cap)
    assert ei.value.code == code and "pg_blend_out_cap" in str(ei.value) and word in str(ei.value)
    L = _lib.load()
    assert len(L.pg_last_error()) > 0
    rows, score = np.zeros((1, max(min(cap, 16), 1)), np.uint64), np.zeros((1, max(min(cap, 16), 1)))
    if 1 <= cap <= 16:                                                  # the host entry point refuses the same, by the same code
        with pytest.raises(PgError) as ei:
            pa.candidates_blend_host(conf, rows, score, np.zeros(rows.shape, np.uint8))
        assert ei.value.code == code


def test_refusals_that_need_the_arrays():
    L = _lib.load()
    conf = engine_conf((REFILL, 4, [(0, 1), (2, 1)]))
    n = 8
    rows, score, source, mask = np.arange(n, dtype=np.uint64), np.zeros(n), np.zeros(n, np.uint8), np.ones(n, np.uint32)
    p64, o64 = np.zeros((3, n)), np.zeros((3, 4))
    o_rows, o_score, o_source, o_mask, o_count = np.zeros(4, np.uint64), np.zeros(4), np.zeros(4, np.uint8), np.zeros(4, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)         # noqa: E731

    def call(src, planes, n64, msk, o_src=o_source, o_pl=o64, o_msk=o_mask, nq=1):
        return L.pg_candidates_blend_host(C.byref(conf), nq, n, p(rows), p(score), p(src), None, p(planes), n64, p(msk), None, 0, p(o_rows),
                                          p(o_score), p(o_src), p(o_pl), p(o_msk), None, p(o_count))
    assert call(source, p64, 3, mask) == 0
    assert call(source, p64, 2, mask) == INVALID and b"n_f64 >= 3" in L.pg_last_error()          # a mask without the planes it needs
    assert call(source, None, 0, mask, o_pl=None) == INVALID and b"planes" in L.pg_last_error()
    assert call(None, None, 0, None, o_src=None, o_pl=None, o_msk=None) == INVALID and b"d_source" in L.pg_last_error()
    assert call(source, None, 0, None, o_pl=None, o_msk=None) == 0                                # neither mask nor planes: legal
    assert call(source, None, 0, None, o_src=None, o_pl=None, o_msk=None) == INVALID and b"pairs" in L.pg_last_error()
    assert call(source, p64, 9, None, o_msk=None) == INVALID and b"1..8 planes" in L.pg_last_error()
    assert call(source, p64, 3, mask, nq=257) == INVALID and b"nq=257" in L.pg_last_error()
    assert L.pg_candidates_blend_host(None, 1, n, p(rows), p(score), None, None, None, 0, None, None, 0, p(o_rows), p(o_score), None, None,
                                      None, None, p(o_count)) == INVALID
    out = C.c_uint32(77)
    assert L.pg_blend_out_cap(None, 10, C.byref(out)) == INVALID and out.value == 77
    assert L.pg_blend_out_cap(C.byref(conf), 10, None) == INVALID
    # the device entry point checks before it touches its context
    assert L.pg_candidates_blend_dev(None, C.byref(conf), 1, n, p(rows), p(score), None, None, None, 0, None, None, 0, p(o_rows), p(o_score),
                                     None, None, None, None, p(o_count)) == INVALID


def engine_conf(conf):
    from pairec_amd.engine import _blend_conf
    return _blend_conf(conf)


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_header_constants_are_the_kernels_and_the_tests():
    with open(os.path.join(ROOT, "include", "pairec_gpu.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "pairec_amd", "csrc", "blend.hip")) as f:
        hip = f.read()
    for macro, const, mine in (("PG_BLEND_MAX_SOURCES", "kBlendMaxSources", ref.MAX_SOURCES), ("PG_BLEND_MAX_PLANES", "kBlendMaxPlanes", ref.MAX_PLANES),
                               ("PG_BLEND_MAX_CAP", "kBlendMaxCap", ref.MAX_CAP)):
        h = re.search(r"#define\s+%s\s+(\d+)" % macro, hdr)
        k = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % const, hip)
        assert h and k and int(h.group(1)) == int(k.group(1)) == mine, macro
    k = re.search(r"constexpr\s+uint32_t\s+kBlendLdsList\s*=\s*(\d+)\s*;", hip)
    assert k and int(k.group(1)) == ref.LDS_LIST
    for macro, mine, engine in (("PG_BLEND_SNAKE_REFILL", REFILL, pa.BLEND_SNAKE_REFILL), ("PG_BLEND_SNAKE_SKIP", SKIP, pa.BLEND_SNAKE_SKIP),
                                ("PG_BLEND_FAIR", FAIR, pa.BLEND_FAIR)):
        h = re.search(r"#define\s+%s\s+(\w+)" % macro, hdr)
        assert h and int(h.group(1), 0) == mine == engine, macro
    # the conf as the binding lays it out: three uint32, eight uint8, eight uint32
    assert C.sizeof(_lib.PgBlendConf) == 52 and _lib.PgBlendConf.source.offset == 12 and _lib.PgBlendConf.weight.offset == 20


# ---- the host mirror's config -------------------------------------------------------------------------------------------------------

MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"feed": {"default": {"RecallNames": ["recall_A", "recall_B", "recall_C"]}}},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": 2000, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
        "Recalls": [{"Name": n, "Kind": "vector", "RecallCount": 50, "RecallAlgo": "gpu_faiss", "ItemType": "video"}
                    for n in ("recall_A", "recall_B", "recall_C", "recall_D")],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "snake", "FilterType": "SnakeFilter", "RetainNum": 20,
                     "AdjustCountConfs": [{"RecallName": "recall_A", "Weight": 1}, {"RecallName": "recall_B", "Weight": 2},
                                          {"RecallName": "recall_C", "Weight": 3}]},
                    {"Name": "snake_skip", "FilterType": "SnakeFilter", "RetainNum": 20, "SnakeType": "SKIP_ON_DUPLICATE",
                     "AdjustCountConfs": [{"RecallName": "recall_C", "Weight": 2}, {"RecallName": "recall_A", "Weight": 0}]},
                    {"Name": "fair", "FilterType": "CompletelyFairCountFilter", "RetainNum": 10}],
        "FilterNames": {"feed": ["snake"]}}},
}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_parse_recconf.restype = C.c_char_p
    L.ph_parse_recconf.argtypes = [C.c_char_p]
    return L


def test_mirror_config_accepts_both_filter_types(H):
    assert H.ph_parse_recconf(json.dumps(MIRROR_CONFIG).encode()), H.ph_last_error()


@pytest.mark.parametrize("edit,words", [
    (lambda f: f[0]["AdjustCountConfs"][1].update({"RecallName": "recall_X"}), (b"pairec_gpu.Filters", b"snake", b'"recall_X"', b"no recall")),
    (lambda f: f[0].update({"RetainNum": 0}), (b"pairec_gpu.Filters", b"snake", b"SnakeFilter", b"retain_num")),
    (lambda f: f[2].pop("RetainNum"), (b"pairec_gpu.Filters", b"fair", b"CompletelyFairCountFilter", b"retain_num")),
    (lambda f: f[0].update({"AdjustCountConfs": []}), (b"pairec_gpu.Filters", b"snake", b"without entries")),
    (lambda f: f[0]["AdjustCountConfs"][2].update({"RecallName": "recall_A"}), (b"pairec_gpu.Filters", b"snake", b"twice")),
    (lambda f: [c.update({"Weight": 0}) for c in f[0]["AdjustCountConfs"]], (b"pairec_gpu.Filters", b"snake", b"every weight is 0")),
    (lambda f: f[1]["AdjustCountConfs"][0].update({"Weight": -1}), (b"pairec_gpu.Filters", b"snake_skip", b"not a count")),
    (lambda f: f[0].update({"AdjustCountConfs": [{"RecallName": "recall_A", "Weight": 1}] * 9}), (b"pairec_gpu.Filters", b"snake", b"9 AdjustCountConfs")),
    (lambda f: f[2].update({"FilterType": "GroupWeightCountFilter"}),
     (b"pairec_gpu.Filters", b'unknown FilterType "GroupWeightCountFilter" (the device serves ItemStateFilter)')),
])
def test_mirror_config_refusals_by_name(H, edit, words):
    cfg = copy.deepcopy(MIRROR_CONFIG)
    edit(cfg["UserDefineConfs"]["pairec_gpu"]["Filters"])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), H.ph_last_error()
