"""CPU checks behind the candidate trim: tests/trim_ref.py — the specification the GPU tests compare with —
against a literal, item-by-item transcription of the reference's loops (filter/priority_adjust_count_filter.go:92-203 without the
diversity branch, filter/adjust_count_filter.go:58-71 without the shuffle); pg_trim_out_cap, the host function that validates a
rule set and sizes the outputs; and the limits the header states against the ones csrc/trim.hip is built with."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import pairec_amd as pa
import trim_ref as ref
from pairec_amd import _lib
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX, ACC, ANY = ref.FIX, ref.ACCUMULATE, ref.ANY
INVALID, UNSUPPORTED = -1, -4


# ---- the reference's loops, item by item --------------------------------------------------------------------------------------------

def go_sort_reverse_by_score(items):
    """sort.Sort(sort.Reverse(psort.ItemScoreSlice(items))) (:92) with the tie order fixed: Less(i, j) = items[j].Score <
    items[i].Score, entries neither of which is Less than the other keep their input order"""
    def cmp(a, b):
        return -1 if b["Score"] < a["Score"] else (1 if a["Score"] < b["Score"] else 0)
    return sorted(items, key=functools.cmp_to_key(cmp))


def go_priority_adjust_count(configs, items):
    """doFilter, ensureDiversity == false; configs = [{RecallName, Type, Count}]"""
    new_items = []
    recall_to_item_map = {}
    items = go_sort_reverse_by_score(items)
    for item in items:                                             # :103-104
        recall_to_item_map.setdefault(item["RetrieveId"], []).append(item)
    accumulator = 0
    for config in configs:                                         # :143
        recall_items = recall_to_item_map.get(config["RecallName"], [])
        if config["Type"] == "fix":
            if len(recall_items) < config["Count"]:
                new_items += recall_items
            else:
                new_items += recall_items[:config["Count"]]
        elif config["Type"] == "accumulator":
            count = config["Count"] - accumulator                  # :193
            assert count >= 0                                      # (Go panics on a negative slice bound)
            if len(recall_items) >= count:
                new_items += recall_items[:count]
                accumulator += count
            else:
                new_items += recall_items
                accumulator += len(recall_items)
    return new_items


def go_adjust_count(retain_num, items):
    """GeneralRank's actions: the ItemRankScore sort, then AdjustCountFilter.doFilter with shuffleItem == false (:58-71)"""
    items = go_sort_reverse_by_score(items)
    if len(items) <= retain_num:
        return items
    return items[:retain_num]


def literal(rules, rows, score, source, count, planes_f64, mask, planes_f32):
    nq, cap = rows.shape
    per_request = []
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        items = [{"pos": i, "Score": float(score[q, i]), "RetrieveId": "s%d" % (source[q, i] if source is not None else 0)}
                 for i in range(n_valid) if int(rows[q, i]) != ref.U64MAX]
        if len(rules) == 1 and rules[0][0] == ANY:
            kept = go_adjust_count(rules[0][2], items)
        else:
            configs = [{"RecallName": "s%d" % s, "Type": "fix" if t == FIX else "accumulator", "Count": c} for s, t, c in rules]
            kept = go_priority_adjust_count(configs, items)
        per_request.append([it["pos"] for it in kept])
    oc = ref.out_cap(rules, cap)
    o_rows = np.full((nq, oc), ref.U64MAX, np.uint64)
    o_score = np.full((nq, oc), ref.NEG_INF_BITS, np.uint64).view(np.float64)
    o_source = None if source is None else np.full((nq, oc), 0xFF, np.uint8)
    o_p64 = np.full((len(planes_f64), nq, oc), ref.NAN_BITS, np.uint64).view(np.float64)
    o_mask = np.zeros((nq, oc), np.uint32)
    o_p32 = np.zeros((len(planes_f32), nq, oc), np.float32)
    o_count = np.zeros(nq, np.uint32)
    for q, kept in enumerate(per_request):
        o_count[q] = len(kept)
        for slot, i in enumerate(kept):
            o_rows[q, slot], o_score[q, slot], o_mask[q, slot] = rows[q, i], score[q, i], mask[q, i]
            if source is not None:
                o_source[q, slot] = source[q, i]
            o_p64[:, q, slot] = planes_f64[:, q, i]
            o_p32[:, q, slot] = planes_f32[:, q, i]
    return o_rows, o_score, o_source, o_p64, o_mask, o_p32, o_count


def heavy_ties(rng, nq, cap, n_src, with_count=True):
    """few distinct scores (±0.0 and the infinities among them), padding sprinkled in, every carried array distinct per entry"""
    values = np.array([-np.inf, -2.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.0, np.inf])
    rows = rng.integers(0, 1 << 40, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < 0.1] = ref.U64MAX
    score = values[rng.integers(0, values.size, (nq, cap))]
    source = rng.integers(0, n_src, (nq, cap)).astype(np.uint8)
    count = rng.integers(0, cap + 1, nq).astype(np.uint32) if with_count else None
    p64 = rng.standard_normal((3, nq, cap))
    mask = rng.integers(0, 256, (nq, cap)).astype(np.uint32)
    p32 = rng.standard_normal((2, nq, cap)).astype(np.float32)
    return rows, score, source, count, p64, mask, p32


RULE_SETS = [
    [(0, FIX, 5)],
    [(2, ACC, 7)],
    [(1, FIX, 4), (0, ACC, 6), (2, ACC, 15)],                       # the reference's documented shape: fix first, then accumulators
    [(0, ACC, 3), (1, FIX, 100), (2, ACC, 3), (3, ACC, 9)],         # an accumulator that is full already, a FIX in between
    [(3, FIX, 0), (1, ACC, 0), (0, ACC, 1000)],
    [(5, FIX, 3), (0, FIX, 2)],                                     # a source without entries (5), sources no rule names
    [(ANY, FIX, 10)], [(ANY, ACC, 10)], [(ANY, FIX, 0)], [(ANY, FIX, 41)],
]


@pytest.mark.parametrize("rules", RULE_SETS)
def test_trim_ref_reads_the_filters_as_their_loops_do(rules):
    rng = np.random.default_rng(len(rules) * 131 + rules[0][2])
    for with_count in (True, False):
        rows, score, source, count, p64, mask, p32 = heavy_ties(rng, 6, 40, 4, with_count)
        ref.same(ref.trim(rules, rows, score, source, count, p64, mask, p32), literal(rules, rows, score, source, count, p64, mask, p32))
    if rules[0][0] == ANY:                                          # ... and without sources at all
        rows, score, _, count, p64, mask, p32 = heavy_ties(rng, 3, 40, 1)
        ref.same(ref.trim(rules, rows, score, None, count, p64, mask, p32), literal(rules, rows, score, None, count, p64, mask, p32))


def test_ties_keep_input_position_and_nan_sorts_last():
    nan = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    score = np.array([[1.0, nan, -0.0, 0.0, 1.0, np.inf, -np.inf, 0.0]])
    rows = np.arange(10, 18, dtype=np.uint64).reshape(1, -1)
    got = ref.trim([(ANY, FIX, 8)], rows, score)
    assert got[0][0].tolist() == [15, 10, 14, 12, 13, 17, 16, 11] and got[6][0] == 8
    assert got[1].view(np.uint64)[0, 7] == 0x7FF8000000000123 and got[1].view(np.uint64)[0, 3] == 0x8000000000000000
    source = np.array([[0, 1, 0, 1, 1, 0, 1, 0]], np.uint8)
    got = ref.trim([(1, FIX, 2), (0, ACC, 3)], rows, score, source)
    assert got[0][0].tolist() == [14, 13, 15, 10, 12] and got[2][0].tolist() == [1, 1, 0, 0, 0]


# ---- pg_trim_out_cap ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rules,cap,want", [
    ([(0, FIX, 5)], 100, 5), ([(0, FIX, 500)], 100, 100), ([(ANY, FIX, 2000)], 8000, 2000), ([(ANY, ACC, 7)], 8000, 7),
    ([(ANY, FIX, 0)], 10, 0), ([(0, FIX, 600), (1, ACC, 1500), (2, ACC, 2000)], 8000, 2600),
    ([(0, ACC, 10), (1, FIX, 3), (2, ACC, 10), (3, FIX, 4)], 16384, 17), ([(7, FIX, 0xFFFFFFFF), (6, FIX, 0xFFFFFFFF)], 16384, 16384),
    ([(s, ACC, 5) for s in range(8)], 1, 1),
])
def test_out_cap(rules, cap, want):
    assert pa.trim_out_cap(rules, cap) == want == ref.out_cap(rules, cap)
    assert pa.Context.trim_out_cap(rules, cap) == want


@pytest.mark.parametrize("rules,cap,code,word", [
    ([], 10, INVALID, "no rules"),
    ([(0, ACC, 10), (1, ACC, 9)], 10, INVALID, "panics"),
    ([(0, ACC, 10), (1, FIX, 50), (2, ACC, 9)], 10, INVALID, "panics"),
    ([(0, FIX, 3), (0, ACC, 9)], 10, INVALID, "twice"),
    ([(ANY, FIX, 3), (0, ACC, 9)], 10, INVALID, "PG_TRIM_ANY"),
    ([(0, FIX, 3), (ANY, FIX, 9)], 10, INVALID, "PG_TRIM_ANY"),
    ([(8, FIX, 3)], 10, INVALID, "source 8"),
    ([(0, 2, 3)], 10, INVALID, "type"),
    ([(s % 8, FIX, 1) for s in range(9)], 10, UNSUPPORTED, "n_rules"),
    ([(0, FIX, 3)], 0, UNSUPPORTED, "cap"),
    ([(0, FIX, 3)], 16385, UNSUPPORTED, "cap"),
])
def test_refused_rule_sets(rules, cap, code, word):
    with pytest.raises(PgError) as ei:
        pa.trim_out_cap(rules, cap)
    assert ei.value.code == code and "pg_trim_out_cap" in str(ei.value) and word in str(ei.value)


def test_out_cap_null_arguments():
    L = _lib.load()
    out = C.c_uint32(77)
    assert L.pg_trim_out_cap(None, 1, 10, C.byref(out)) == INVALID and out.value == 77
    arr = (_lib.PgTrimRule * 1)(_lib.PgTrimRule(0, FIX, 3))
    assert L.pg_trim_out_cap(arr, 1, 10, None) == INVALID


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_header_constants_are_the_kernels_and_the_tests():
    with open(os.path.join(ROOT, "include", "pairec_gpu.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "pairec_amd", "csrc", "trim.hip")) as f:
        hip = f.read()
    for macro, const, mine in (("PG_TRIM_MAX_RULES", "kTrimMaxRules", ref.MAX_RULES), ("PG_TRIM_MAX_SOURCES", "kTrimMaxSources", ref.MAX_SOURCES),
                               ("PG_TRIM_MAX_PLANES", "kTrimMaxPlanes", ref.MAX_PLANES), ("PG_TRIM_MAX_CAP", "kTrimMaxCap", ref.MAX_CAP),
                               ("PG_TRIM_CHUNK", "kTrimChunk", ref.CHUNK)):
        h = re.search(r"#define\s+%s\s+(\d+)" % macro, hdr)
        k = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % const, hip)
        assert h and k and int(h.group(1)) == int(k.group(1)) == mine, macro
    for macro, mine, engine in (("PG_TRIM_FIX", FIX, pa.TRIM_FIX), ("PG_TRIM_ACCUMULATE", ACC, pa.TRIM_ACCUMULATE), ("PG_TRIM_ANY", ANY, pa.TRIM_ANY)):
        h = re.search(r"#define\s+%s\s+(\w+)" % macro, hdr)
        assert h and int(h.group(1), 0) == mine == engine, macro
    # the rule as the binding lays it out: uint8, uint8, two bytes of padding, uint32
    assert re.search(r"uint8_t\s+source;.*\n\s*uint8_t\s+type;.*\n\s*uint32_t\s+count;", hdr)
    assert C.sizeof(_lib.PgTrimRule) == 8 and _lib.PgTrimRule.count.offset == 4 and _lib.PgTrimRule.type.offset == 1
