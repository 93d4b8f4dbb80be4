"""CPU checks behind PriorityAdjustCountFilterV2 on the device: the reference's own three test cases
(tests/golden/priority_adjust_count_v2.json) through fanin_ref + trim2_ref and through pg_candidates_trim2_host; trim2_ref's array
statement against its item-by-item transcription of the Go loop (filter/priority_adjust_count_filter_v2.go:39-103) where the
reference is deterministic; pg_candidates_trim2_host, the library's host statement, against the array statement by bits;
pg_trim2_out_cap and every refusal; and the host mirror's config parse for both quota filters."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import fanin_ref
import trim2_ref as ref
import trim_ref
import pairec_amd as pa
from pairec_amd import _lib
from pairec_amd._lib import PgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX, ACC, ANY = ref.FIX, ref.ACCUMULATE, ref.ANY
INVALID, UNSUPPORTED = -1, -4
with open(os.path.join(ROOT, "tests", "golden", "priority_adjust_count_v2.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
TYPES = {"fix": FIX, "accumulator": ACC}


# ---- the reference's own cases ------------------------------------------------------------------------------------------------------

def golden_merge(case):
    """the case's input list → (id names by row, rules, the arrays fanin_ref leaves): one fan-in source per recall, in the order
    the recalls first appear in the list, so that the concatenation is the list"""
    recalls = case["recalls"]
    names = []
    for it in case["items"]:
        if it[0] not in names:
            names.append(it[0])
    width = max(sum(1 for it in case["items"] if it[2] == r) for r in recalls)
    sources = []
    for r in recalls:
        mine = [it for it in case["items"] if it[2] == r]
        rows = np.full((1, width), ref.U64MAX, np.uint64)
        sc = np.zeros((1, width))
        rows[0, :len(mine)] = [names.index(it[0]) for it in mine]
        sc[0, :len(mine)] = [it[1] for it in mine]
        sources.append((rows, sc))
    rules = [(recalls.index(c["RecallName"]), TYPES[c["Type"]], c["Count"]) for c in case["confs"]]
    return names, rules, fanin_ref.merge(sources)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_the_reference_tests_answers(case):
    names, rules, (rows, score, source, planes, mask, count) = golden_merge(case)
    n = len(case["expect_ids"])
    want_rows = [names.index(i) for i in case["expect_ids"]]
    want_src = [case["recalls"].index(r) for r in case["expect_retrieve_ids"]]
    for got in (ref.trim2(rules, rows, score, source, count, planes, mask),
                pa.candidates_trim2_host(rules, rows, score, source, count, planes, mask)):
        assert got[6][0] == n == len(want_src)
        assert got[0][0, :n].tolist() == want_rows and got[2][0, :n].tolist() == want_src
        assert (got[0][0, n:] == ref.U64MAX).all()
    # ... and through the transcription of the loop, on objects, UniqueFilter included where the test runs it
    items = [ref.Item(i, s, r) for i, s, r in case["items"]]
    if case["unique_filter"]:
        items = ref.unique_filter(items)
    kept = ref.go_v2(case["confs"], items)
    assert [it.Id for it in kept] == case["expect_ids"] and [it.RetrieveId for it in kept] == case["expect_retrieve_ids"]
    if case["name"] == "AccumulateCount_Unique":
        assert kept[0].Score == 11.0 and got[1][0, 0] == 11.0               # the pick leaves with u2i's score, not hot's -1


def test_golden_fixture_is_data_with_citations():
    assert [c["name"] for c in GOLDEN] == ["FixCount", "AccumulateCount", "AccumulateCount_Unique"]
    assert [len(c["expect_ids"]) for c in GOLDEN] == [10, 15, 15]
    assert GOLDEN[2]["expect_ids"][0] == "item_a&b" and GOLDEN[2]["expect_retrieve_ids"][0] == "u2i"
    for c in GOLDEN:
        assert re.match(r"filter/priority_adjust_count_filter_v2_test\.go:\d+-\d+$", c["cites"]), c["name"]


# ---- random merges --------------------------------------------------------------------------------------------------------------------

NAN_PAYLOAD = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
VALUES = np.array([-np.inf, -2.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.0, np.inf, NAN_PAYLOAD, 5e-324, -5e-324])


def merged(rng, nq, cap, n_src, with_count=True, overlap=0.4, values=VALUES, distinct=False):
    """what a fan-in could have left: few distinct scores (±0.0, infinities, NaN and subnormals among them), padding sprinkled in
    the middle, sources past the limit, masks that name the first source and some others, every carried array distinct;
    distinct: every key a number of its own"""
    rows = rng.permutation(nq * cap).reshape(nq, cap).astype(np.uint64) + np.uint64(1 << 33)
    rows[rng.random((nq, cap)) < 0.08] = ref.U64MAX
    source = rng.integers(0, n_src, (nq, cap)).astype(np.uint8)
    source[rng.random((nq, cap)) < 0.03] = 9                        # (a source no rule can name)
    count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32) if with_count else None
    if distinct:
        all_keys = rng.permutation((n_src + 1) * nq * cap).astype(np.float64).reshape(n_src + 1, nq, cap) * 0.5 - 7.0
        score, p64 = all_keys[0], all_keys[1:]
    else:
        score = values[rng.integers(0, values.size, (nq, cap))]
        p64 = values[rng.integers(0, values.size, (n_src, nq, cap))]
    others = np.zeros((nq, cap), np.uint32)
    for b in range(n_src):
        others |= (rng.random((nq, cap)) < overlap).astype(np.uint32) << np.uint32(b)
    mask = (others | (np.uint32(1) << (source.astype(np.uint32) & 31))).astype(np.uint32)
    p32 = rng.standard_normal((2, nq, cap)).astype(np.float32)
    return rows, score, source, count, p64, mask, p32


def random_rules(rng, n_src, cap, decreasing=True):
    named = rng.permutation(n_src)[:int(rng.integers(1, n_src + 1))]
    rules, top = [], 0
    for s in named:
        typ = int(rng.integers(0, 2))
        cnt = int(rng.choice([0, 1, 2, cap // 4, cap // 2, cap, cap + 7, 0xFFFFFFFF]))
        if typ == ACC and not decreasing:
            cnt = max(cnt, top)
            top = cnt
        rules.append((int(s), typ, cnt))
    return rules


def random_cases(n, seed, distinct=False, decreasing=True):
    rng = np.random.default_rng(seed)
    for k in range(n):
        n_src = int(rng.integers(1, 7))
        cap = int(rng.integers(1, 70))
        data = merged(rng, 2, cap, n_src, with_count=bool(k % 2), overlap=float(rng.choice([0.0, 0.3, 1.0])), distinct=distinct)
        yield random_rules(rng, n_src, cap, decreasing), data


def literal(rules, rows, score, source, count, p64, mask, p32):
    """the transcription over the same arrays: items are built as the fan-in's outputs describe them (RetrieveId = the source,
    RecallScores = the planes the mask names), the filter runs on objects, and what it returns is written out"""
    nq, cap = rows.shape
    oc = ref.out_cap(rules, cap)
    o_rows = np.full((nq, oc), ref.U64MAX, np.uint64)
    o_score = np.full((nq, oc), ref.NEG_INF_BITS, np.uint64).view(np.float64)
    o_source = np.full((nq, oc), 0xFF, np.uint8)
    o_p64 = np.full((len(p64), nq, oc), ref.NAN_BITS, np.uint64).view(np.float64)
    o_mask = None if mask is None else np.zeros((nq, oc), np.uint32)
    o_p32 = np.zeros((len(p32), nq, oc), np.float32)
    o_count = np.zeros(nq, np.uint32)
    confs = [{"RecallName": "s%d" % s, "Type": "fix" if t == FIX else "accumulator", "Count": c} for s, t, c in rules]
    for q in range(nq):
        n_valid = cap if count is None else min(int(count[q]), cap)
        items = []
        for i in range(n_valid):
            if int(rows[q, i]) == ref.U64MAX:
                continue
            scores = {}
            if mask is not None:
                scores = {"s%d" % b: (p64[b, q, i] if b < len(p64) else 0.0) for b in range(32) if (int(mask[q, i]) >> b) & 1}
            items.append(ref.Item(i, score[q, i], "s%d" % source[q, i], scores))
        kept = ref.go_v2(confs, items)
        o_count[q] = len(kept)
        for slot, it in enumerate(kept):
            i = it.Id
            o_rows[q, slot], o_score[q, slot], o_source[q, slot] = rows[q, i], it.Score, int(it.RetrieveId[1:])
            if mask is not None:
                o_mask[q, slot] = mask[q, i]
            o_p64[:, q, slot] = p64[:, q, i]
            o_p32[:, q, slot] = p32[:, q, i]
    return o_rows, o_score, o_source, o_p64, o_mask, o_p32, o_count


def test_trim2_ref_reads_the_filter_as_its_loop_does():
    # keys distinct inside every list: there the reference's shuffle and unstable sort decide nothing
    n_dup = 0
    for rules, (rows, score, source, count, p64, mask, p32) in random_cases(300, 51, distinct=True):
        want = literal(rules, rows, score, source, count, p64, mask, p32)
        ref.same(ref.trim2(rules, rows, score, source, count, p64, mask, p32), want)
        n_dup += int((want[2] != 0xFF).sum())
    assert n_dup > 1000
    # (with ties the transcription appends the duplicates behind the singles before it sorts, so equal keys come out in that
    # order and not by input position: the one place where the definition fixes what the reference leaves to chance)
    # without a mask nothing is reached through a second recall, and ties keep input position in both
    for rules, (rows, score, source, count, p64, _, p32) in random_cases(40, 53):
        ref.same(ref.trim2(rules, rows, score, source, count, p64, None, p32), literal(rules, rows, score, source, count, p64, None, p32))


def test_host_statement_equals_trim2_ref_by_bits():
    for rules, (rows, score, source, count, p64, mask, p32) in random_cases(300, 51):
        ref.same(pa.candidates_trim2_host(rules, rows, score, source, count, p64, mask, p32),
                 ref.trim2(rules, rows, score, source, count, p64, mask, p32))
    for rules, (rows, score, source, count, p64, mask, p32) in random_cases(60, 54):
        for kw in ({}, {"source": source}, {"count": count}, {"planes_f64": p64}, {"planes_f32": p32},
                   {"planes_f64": p64, "source_mask": mask}, {"source": source, "planes_f64": p64, "source_mask": mask}):
            r = rules if "source" in kw else rules[:1]                  # (without sources one rule owns every entry)
            ref.same(pa.candidates_trim2_host(r, rows, score, **kw), ref.trim2(r, rows, score, **kw))


def test_without_a_mask_the_answer_is_the_trims():
    n = 0
    for rules, (rows, score, source, count, p64, mask, p32) in random_cases(200, 55, decreasing=False):
        want = trim_ref.trim(rules, rows, score, source, count, p64, None, p32)
        ref.same(pa.candidates_trim2_host(rules, rows, score, source, count, p64, None, p32), want)
        ref.same(ref.trim2(rules, rows, score, source, count, p64, None, p32), want)
        n += int(want[6].sum())
    assert n > 500


def test_ties_nan_the_rewrite_and_the_places():
    # two recalls; item 12 stands in both lists: first in recall 0 (score 1.0), recall 1 scores it 9.0; 11 has a NaN score
    rows = np.arange(10, 16, dtype=np.uint64).reshape(1, -1)
    score = np.array([[2.0, NAN_PAYLOAD, 1.0, -0.0, 0.0, 5.0]])
    source = np.array([[0, 0, 0, 1, 1, 1]], np.uint8)
    mask = np.array([[1, 1, 3, 2, 2, 2]], np.uint32)
    p64 = np.full((2, 1, 6), np.nan)
    p64[0, 0, :3], p64[1, 0, 3:], p64[1, 0, 2] = score[0, :3], score[0, 3:], 9.0
    # lists: recall 0 = 10 (2.0), 12 (1.0), 11 (NaN); recall 1 = 12 (9.0), 15 (5.0), 13 (-0.0), 14 (0.0): ±0 tie by position
    got = ref.trim2([(1, FIX, 2), (0, FIX, 2)], rows, score, source, None, p64, mask)
    # 12 leaves through recall 1 and does not use up a place of recall 0: 10 and then 11
    assert got[0][0].tolist() == [12, 15, 10, 11] and got[2][0].tolist() == [1, 1, 0, 0] and got[6][0] == 4
    assert got[1][0, 0] == 9.0 and got[1].view(np.uint64)[0, 3] == 0x7FF8000000000123
    ref.same(pa.candidates_trim2_host([(1, FIX, 2), (0, FIX, 2)], rows, score, source, None, p64, mask), got)
    got = ref.trim2([(0, ACC, 2), (1, ACC, 5)], rows, score, source, None, p64, mask)
    assert got[0][0].tolist() == [10, 12, 15, 13, 14] and got[1][0, 1] == 1.0 and got[1].view(np.uint64)[0, 3] == 1 << 63
    ref.same(pa.candidates_trim2_host([(0, ACC, 2), (1, ACC, 5)], rows, score, source, None, p64, mask), got)
    # a decreasing accumulate count is a limit of 0, not an error; a FIX rule between leaves the accumulator alone
    got = pa.candidates_trim2_host([(0, ACC, 2), (1, ACC, 1)], rows, score, source, None, p64, mask)
    assert got[0][0].tolist() == [10, 12] and got[6][0] == 2
    # a duplicate's own plane is its key in its own recall's list as well: the id came twice in recall 0 (plane 7.0, score 1.0)
    p64[0, 0, 2] = 7.0
    got = pa.candidates_trim2_host([(0, FIX, 1)], rows, score, source, None, p64, mask)
    assert got[0][0].tolist() == [12] and got[1][0, 0] == 7.0
    ref.same(got, ref.trim2([(0, FIX, 1)], rows, score, source, None, p64, mask))


# ---- pg_trim2_out_cap and the refusals ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rules,cap,want", [
    ([(0, FIX, 5)], 100, 5), ([(0, FIX, 5), (3, ACC, 500)], 100, 100), ([(2, ACC, 1500), (0, FIX, 600), (1, ACC, 2000)], 8000, 2600),
    ([(0, ACC, 7), (1, ACC, 3)], 100, 7),                                        # decreasing accumulate counts are legal here
    ([(s, FIX, 0xFFFFFFFF) for s in range(8)], 16384, 16384),                     # the sum is taken in 64 bits
    ([(0, FIX, 0xFFFFFFFF), (1, ACC, 0xFFFFFFFF), (2, FIX, 2)], 9, 9), ([(0, FIX, 0), (1, ACC, 0)], 50, 0), ([(7, ACC, 1)], 1, 1),
])
def test_out_cap(rules, cap, want):
    assert pa.trim2_out_cap(rules, cap) == want == ref.out_cap(rules, cap)
    assert pa.Context.trim2_out_cap(rules, cap) == want


REFUSED = [
    ([], 10, INVALID, "no rules"),
    ([(0, FIX, 1), (1, ACC, 2), (0, FIX, 3)], 10, INVALID, "twice"),
    ([(ANY, FIX, 5)], 10, INVALID, "PG_TRIM_ANY"),
    ([(0, FIX, 5), (ANY, FIX, 5)], 10, INVALID, "PG_TRIM_ANY"),
    ([(8, ACC, 5)], 10, INVALID, "source 8"),
    ([(0, 2, 5)], 10, INVALID, "type 2"),
    ([(s % 8, FIX, 1) for s in range(9)], 10, UNSUPPORTED, "n_rules"),
    ([(0, FIX, 1)], 0, UNSUPPORTED, "cap"),
    ([(0, FIX, 1)], 16385, UNSUPPORTED, "cap"),
]


@pytest.mark.parametrize("rules,cap,code,word", REFUSED)
def test_refused_rules(rules, cap, code, word):
    with pytest.raises(PgError) as ei:
        pa.trim2_out_cap(rules, cap)
    assert ei.value.code == code and "pg_trim2_out_cap" in str(ei.value) and word in str(ei.value)
    assert len(_lib.load().pg_last_error()) > 0
    rows, score = np.zeros((1, max(min(cap, 16), 1)), np.uint64), np.zeros((1, max(min(cap, 16), 1)))
    if 1 <= cap <= 16:                                                  # the host entry point refuses the same, by the same code
        with pytest.raises(PgError) as ei:
            pa.candidates_trim2_host(rules, rows, score, np.zeros(rows.shape, np.uint8))
        assert ei.value.code == code and word in str(ei.value)
        from pairec_amd.engine import _trim_rules
        o = np.zeros((1, 16), np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                        # noqa: E731
        rc = _lib.load().pg_candidates_trim2_host(_trim_rules(rules), len(rules), 1, rows.shape[1], p(rows), p(score), None, None, None, 0,
                                                  None, None, 0, p(o), p(o.view(np.float64).copy()), None, None, None, None,
                                                  p(np.zeros(1, np.uint32)))
        assert rc == code and b"pg_candidates_trim2_host" in _lib.load().pg_last_error() and word.encode() in _lib.load().pg_last_error()


def test_refusals_that_need_the_arrays():
    from pairec_amd.engine import _trim_rules
    L = _lib.load()
    rules = _trim_rules([(0, FIX, 2), (2, ACC, 4)])
    n = 8
    rows, score, source, mask = np.arange(n, dtype=np.uint64), np.zeros(n), np.zeros(n, np.uint8), np.ones(n, np.uint32)
    p64, o64 = np.zeros((3, n)), np.zeros((3, 6))
    o_rows, o_score, o_source, o_mask, o_count = np.zeros(6, np.uint64), np.zeros(6), np.zeros(6, np.uint8), np.zeros(6, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)         # noqa: E731

    def call(src, planes, n64, msk, o_src=o_source, o_pl=o64, o_msk=o_mask, nq=1, n_rules=2, o_r=o_rows):
        return L.pg_candidates_trim2_host(rules, n_rules, nq, n, p(rows), p(score), p(src), None, p(planes), n64, p(msk), None, 0, p(o_r),
                                          p(o_score), p(o_src), p(o_pl), p(o_msk), None, p(o_count))
    assert call(source, p64, 3, mask) == 0
    assert call(source, p64, 2, mask) == INVALID and b"n_f64 >= 3" in L.pg_last_error()          # a mask without the planes it needs
    assert call(source, None, 0, mask, o_pl=None) == INVALID and b"planes" in L.pg_last_error()
    assert call(None, None, 0, None, o_src=None, o_pl=None, o_msk=None) == INVALID and b"d_source" in L.pg_last_error()
    assert call(None, None, 0, None, o_src=None, o_pl=None, o_msk=None, n_rules=1) == 0          # one rule owns every entry
    assert call(source, None, 0, None, o_pl=None, o_msk=None) == 0                                # neither mask nor planes: legal
    assert call(source, None, 0, None, o_src=None, o_pl=None, o_msk=None) == INVALID and b"pairs" in L.pg_last_error()
    assert call(source, p64, 3, None, o_pl=None, o_msk=None) == INVALID and b"pairs" in L.pg_last_error()
    assert call(source, p64, 9, None, o_msk=None) == INVALID and b"1..8 planes" in L.pg_last_error()
    assert call(source, p64, 3, mask, nq=257) == INVALID and b"nq=257" in L.pg_last_error()
    assert call(source, p64, 3, mask, o_r=rows) == INVALID and b"overlaps" in L.pg_last_error()
    assert call(source, p64, 3, mask, o_pl=p64[1:]) == INVALID and b"overlaps" in L.pg_last_error()
    assert call(source, p64, 3, mask) == 0
    assert L.pg_candidates_trim2_host(None, 1, 1, n, p(rows), p(score), None, None, None, 0, None, None, 0, p(o_rows), p(o_score), None, None,
                                      None, None, p(o_count)) == INVALID
    out = C.c_uint32(77)
    assert L.pg_trim2_out_cap(None, 1, 10, C.byref(out)) == INVALID and out.value == 77
    assert L.pg_trim2_out_cap(rules, 2, 10, None) == INVALID
    # the device entry point checks before it touches its context
    assert L.pg_candidates_trim2_dev(None, rules, 2, 1, n, p(rows), p(score), None, None, None, 0, None, None, 0, p(o_rows), p(o_score),
                                     None, None, None, None, p(o_count)) == INVALID


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_header_and_sources_name_the_call():
    with open(os.path.join(ROOT, "include", "pairec_gpu.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "pairec_amd", "csrc", "trim2.hip")) as f:
        hip = f.read()
    for name in ("pg_trim2_out_cap", "pg_candidates_trim2_dev", "pg_candidates_trim2_host"):
        assert re.search(r"\bint %s\(" % name, hdr) and re.search(r"\bint %s\(" % name, hip), name
        assert hasattr(_lib.load(), name)
    for macro, const, mine in (("PG_TRIM_MAX_RULES", "kTrim2MaxRules", ref.MAX_RULES), ("PG_TRIM_CHUNK", "kTrim2Chunk", ref.CHUNK)):
        h = re.search(r"#define\s+%s\s+(\d+)" % macro, hdr)
        k = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % const, hip)
        assert h and k and int(h.group(1)) == int(k.group(1)) == mine, macro
    assert "kSlotTrim2" in hip
    assert (FIX, ACC, ANY) == (pa.TRIM_FIX, pa.TRIM_ACCUMULATE, pa.TRIM_ANY)


# ---- the host mirror's config -------------------------------------------------------------------------------------------------------

MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"feed": {"default": {"RecallNames": ["recall_A", "recall_B", "recall_C"]}}},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": 2000, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
        "Recalls": [{"Name": n, "Kind": "vector", "RecallCount": 50, "RecallAlgo": "gpu_faiss", "ItemType": "video"}
                    for n in ("recall_A", "recall_B", "recall_C", "recall_D")],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "quota2", "FilterType": "PriorityAdjustCountFilterV2",
                     "AdjustCountConfs": [{"RecallName": "recall_B", "Count": 10, "Type": "accumulator"},
                                          {"RecallName": "recall_A", "Count": 5, "Type": "fix"},
                                          {"RecallName": "recall_C", "Count": 4, "Type": "accumulator"}]},
                    {"Name": "quota1", "FilterType": "PriorityAdjustCountFilter",
                     "AdjustCountConfs": [{"RecallName": "recall_C", "Count": 10, "Type": "accumulator"},
                                          {"RecallName": "recall_A", "Count": 20, "Type": "accumulator"}]}],
        "FilterNames": {"feed": ["quota2", "quota1"]}}},
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


V2, V1 = b"PriorityAdjustCountFilterV2", b"PriorityAdjustCountFilter"


@pytest.mark.parametrize("edit,words", [
    (lambda f: f[0]["AdjustCountConfs"][1].update({"RecallName": "recall_X"}), (b"pairec_gpu.Filters", b"quota2", V2, b'"recall_X"', b"no recall")),
    (lambda f: f[1]["AdjustCountConfs"][1].update({"RecallName": "recall_X"}), (b"pairec_gpu.Filters", b"quota1", V1, b'"recall_X"', b"no recall")),
    (lambda f: f[0].update({"AdjustCountConfs": []}), (b"pairec_gpu.Filters", b"quota2", V2, b"AdjustCountConfs is empty")),
    (lambda f: f[1].pop("AdjustCountConfs"), (b"pairec_gpu.Filters", b"quota1", V1, b"AdjustCountConfs is empty")),
    (lambda f: f[0]["AdjustCountConfs"][2].update({"RecallName": "recall_B"}), (b"pairec_gpu.Filters", b"quota2", V2, b"twice")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Count": -1}), (b"pairec_gpu.Filters", b"quota2", V2, b'Count of "recall_B"', b"not a count")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Count": 2.5}), (b"pairec_gpu.Filters", b"quota2", V2, b"not a count")),
    (lambda f: f[0]["AdjustCountConfs"][0].update({"Count": "7"}), (b"pairec_gpu.Filters", b"quota2", V2, b"not a count")),
    (lambda f: f[1]["AdjustCountConfs"][0].pop("Count"), (b"pairec_gpu.Filters", b"quota1", V1, b"not a count")),
    (lambda f: f[0]["AdjustCountConfs"][1].update({"Type": "weight"}), (b"pairec_gpu.Filters", b"quota2", V2, b'Type "weight"', b"fix and accumulator")),
    (lambda f: f[1]["AdjustCountConfs"][1].pop("Type"), (b"pairec_gpu.Filters", b"quota1", V1, b'Type ""')),
    (lambda f: f[0].update({"AdjustCountConfs": [{"RecallName": "recall_A", "Count": 1, "Type": "fix"}] * 9}),
     (b"pairec_gpu.Filters", b"quota2", V2, b"9 AdjustCountConfs")),
    # v1 slices with a negative bound where its accumulate counts decrease; V2 (quota2 above: 10 then 4) compares and is served
    (lambda f: f[1]["AdjustCountConfs"][1].update({"Count": 3}), (b"pairec_gpu.Filters", b"quota1", V1, b"accumulates to 3 after 10")),
    (lambda f: f[1].update({"EnsureDiversity": True}), (b"pairec_gpu.Filters", b"quota1", V1, b"EnsureDiversity", b"diversity branch")),
    (lambda f: f[1].update({"DiversityMinCount": 2}), (b"pairec_gpu.Filters", b"quota1", V1, b"DiversityMinCount", b"diversity branch")),
    (lambda f: f[1].update({"DiversityDaoConf": {"AdapterType": "hologres"}}), (b"pairec_gpu.Filters", b"quota1", V1, b"DiversityDaoConf")),
    (lambda f: f[1].update({"FilterType": "GroupWeightCountFilter"}),
     (b"pairec_gpu.Filters", b'unknown FilterType "GroupWeightCountFilter" (the device serves ItemStateFilter)')),
])
def test_mirror_config_refusals_by_name(H, edit, words):
    cfg = copy.deepcopy(MIRROR_CONFIG)
    edit(cfg["UserDefineConfs"]["pairec_gpu"]["Filters"])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), H.ph_last_error()


def test_mirror_recall_past_the_eighth_is_refused_by_name(H):
    cfg = copy.deepcopy(MIRROR_CONFIG)
    gpu = cfg["UserDefineConfs"]["pairec_gpu"]
    gpu["Recalls"] = [dict(gpu["Recalls"][0], Name="recall_%d" % i) for i in range(9)]
    gpu["Filters"] = [{"Name": "q", "FilterType": "PriorityAdjustCountFilterV2",
                       "AdjustCountConfs": [{"RecallName": "recall_8", "Count": 1, "Type": "fix"}]}]
    cfg["SceneConfs"]["feed"]["default"]["RecallNames"] = ["recall_0"]
    gpu["FilterNames"] = {"feed": ["q"]}
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    assert b'"recall_8" is recall 8' in H.ph_last_error() and V2 in H.ph_last_error()
