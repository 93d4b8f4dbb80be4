"""CPU tests of the list recall (csrc/hot_host.hpp behind pg_hot_recall_host): the host statement against
tests/hot_ref.py over the whole grid of tests/hot_cases.py and the hand-derived answers of tests/golden/hot_known_answers.json —
rows, counts and sources as integers, scores as bit patterns —, the refusals of requests and of tables (pg_hot_recall_host holds
its CSR to what pg_hottable_upload accepts: the same validation), and the binding's constants."""
import json
import os
import re

import numpy as np
import pytest

import hot_cases as cases
import hot_ref as ref
import pairec_amd as pa
from pairec_amd._lib import PgError

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = -1, -4


def host(mode, trig, k, values=None, seed=None, tab=None):
    off, rows, sc, src = tab or cases.table()[1]
    return pa.hot_recall_host(cases.ROWS, cases.ROW_OFFSET, off, rows, sc, src, mode, trig, k, values, seed)


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(HERE), "include", "pairec_gpu.h")).read()
    for name in ("GROUP", "GLOBAL", "TOPIC", "MAX_ENTRIES", "UNSCORED", "PAD_SOURCE"):
        m = re.search(r"#define PG_HOT_%s (\w+)" % name, text)
        assert m and int(m.group(1).rstrip("u"), 0) == getattr(pa, "HOT_" + name) == getattr(ref, name), name


@pytest.mark.parametrize("name", sorted(cases.grid()))
def test_grid(name):
    mode, trig, values, seed, k = cases.grid()[name]
    want = cases.expected(name)
    got = host(mode, trig, k, values, seed)
    ref.same(got, want)
    if "empty_and_absent" in name:
        assert not want[3].any() and np.all(want[2] == ref.PAD_SOURCE) and np.all(np.isneginf(want[1]))
    if name.endswith("k_above_n"):
        assert want[3][0] == 63 and np.all(want[0][0, 63:] == ref.PAD_ROW) and np.all(want[2][0, 63:] == 0xFF)
    if name == "global_workgroup_edges":
        off, rows = cases.table()[1][:2]
        stored = cases.ROW_OFFSET + rows[int(off[cases.T_1024]):int(off[cases.T_1024 + 1])].astype(np.uint64)
        assert np.array_equal(want[0][1], stored)                        # n == k: the stored order, draws included
        assert np.all(np.diff(want[1][2]) <= 0) and not np.all(np.diff(want[1][1]) <= 0)    # n == k + 1: sorted
    if name.endswith("ties_across_lists") or name.endswith("ties_across_tier_edge"):
        n = int(want[3][0])
        assert len(set(want[1][0, :n].tolist())) == 1                    # all scores equal: the order is the position
        off, rows = cases.table()[1][:2]
        cat = np.concatenate([rows[int(off[t]):int(off[t + 1])] for t in trig[0]])
        assert np.array_equal(want[0][0, :n], cases.ROW_OFFSET + cat[:n].astype(np.uint64))
    if name == "group_special_scores":
        sc = want[1][0, :int(want[3][0])]
        assert np.signbit(sc[sc == 0]).any() and not np.signbit(sc[sc == 0]).all()          # -0.0 beside 0.0, bits kept
        assert 16777217.0 in sc and 5e-324 in sc and -1.7e308 == sc[-1] and 1.7e308 == sc[0]
    if name.endswith("_sources"):
        assert set(want[2][0, :6].tolist()) == {0, 1, 126}               # bit 7 is stripped
    if name == "topic_zero_is_half":
        assert want[3][0] == 9 and ref.topic_quotas([0.0, 1.5], 10) == [2, 7]
    if name == "topic_sum_below_k":
        assert want[3][0] == 999
    if name == "topic_huge_values":
        assert list(want[3]) == [0, 100]


def test_draws_are_the_formula():
    mode, trig, values, seed, k = cases.grid()["global_all_unscored_k300"]
    got = host(mode, trig, k, values, seed)
    for q in range(2):
        assert [float(x) for x in got[1][q]] == [ref.draw(seed[q], p) for p in range(300)]
    assert ref.draw(0, 0) == float(0xE220A8397B1DCDAF >> 11) * 2.0 ** -53   # splitmix64's first output from state 0
    no_seed = host(GLOBAL, [[cases.T_UNSCORED]], 300)
    assert np.array_equal(no_seed[1][0].view(np.uint64), got[1][0].view(np.uint64))          # NULL = 0


GLOBAL = ref.GLOBAL


def test_known_answers():
    with open(os.path.join(HERE, "golden", "hot_known_answers.json")) as f:
        gold = json.load(f)
    row_of = {name: i for i, name in enumerate(gold["items"])}
    source_of = {name: i for i, name in enumerate(gold["sources"])}
    modes = {"group": ref.GROUP, "global": ref.GLOBAL, "topic": ref.TOPIC}
    assert len(gold["cases"]) >= 5
    for c in gold["cases"]:
        names = sorted(c["lists"])
        parsed = [ref.parse_item_ids(c["lists"][n], row_of, source_of) for n in names]
        off = np.zeros(len(names) + 1, np.uint64)
        off[1:] = np.cumsum([len(p[0]) for p in parsed])
        rows, sc, src = (np.concatenate([p[i] for p in parsed]) for i in range(3))
        trig = [[names.index(n) for n in c["request"]]]
        values = None
        if "values" in c:                                              # user_topic_mysql_dao.go:70-84: "topic:value,..."
            pairs = dict(tv.split(":") for tv in c["values"].split(","))
            values = [[float(pairs[n]) for n in c["request"]]]
        seed = [c["seed"]] if "seed" in c else None
        k, n = c["k"], len(c["expect_ids"])
        want_sc = [ref.draw(c["seed"], p) if s is None else s for p, s in enumerate(c["expect_scores"])]
        for got in (pa.hot_recall_host(len(row_of), 0, off, rows, sc, src, modes[c["mode"]], trig, k, values, seed),
                    ref.recall(len(row_of), 0, off, rows, sc, src, modes[c["mode"]], trig, k, values, seed)):
            assert got[3][0] == n, c["name"]
            assert [gold["items"][int(r)] for r in got[0][0, :n]] == c["expect_ids"], c["name"]
            assert [float(x) for x in got[1][0, :n]] == want_sc, c["name"]
            assert [gold["sources"][int(s)] for s in got[2][0, :n]] == c["expect_sources"], c["name"]
            assert np.all(got[0][0, n:] == ref.PAD_ROW) and np.all(got[2][0, n:] == 0xFF)
    # the arithmetic the topic case rests on
    assert int(0.25 * 10) == 2 and int(0.75 * 10) == 7 and (0.5 / 2.0) * 10.0 == 2.5 and (1.5 / 2.0) * 10.0 == 7.5


def test_parse_item_ids():
    rows, sc, src = ref.parse_item_ids("a,b:,c:x,d:x:1.5,e::2,,f:y:zz,g:x:1:9", {c: i for i, c in enumerate("abcdefg")}, {"x": 1, "y": 126})
    assert rows.tolist() == [0, 1, 2, 3, 4, 5] and sc.tolist() == [0, 0, 0, 1.5, 2, 0]
    assert src.tolist() == [0x80, 0x80, 0x81, 1, 0, 126]


def refused(code, match, fn, *a, **kw):
    with pytest.raises(PgError) as e:
        fn(*a, **kw)
    assert e.value.code == code and re.search(match, str(e.value)), str(e.value)


def test_request_refusals():
    for trig, q in cases.TOO_LONG:
        refused(UNSUPPORTED, r"request %d concatenates 65537 entries" % q, host, ref.GROUP, trig, 10)
        with pytest.raises(ref.Unsupported) as e:
            cases_off, rows, sc, src = cases.table()[1]
            ref.recall(cases.ROWS, cases.ROW_OFFSET, cases_off, rows, sc, src, ref.GROUP, trig, 10)
        assert e.value.request == q
    ref.same(host(ref.TOPIC, [[cases.T_MAX, cases.T_EXTRA]], 16384, [[1.0, 1.0]]),           # quotas keep a topic request within k
             ref.recall(cases.ROWS, cases.ROW_OFFSET, *cases.table()[1], ref.TOPIC, [[cases.T_MAX, cases.T_EXTRA]], 16384, [[1.0, 1.0]]))
    refused(INVALID, "mode 3", host, 3, [[1]], 10)
    refused(INVALID, "mode -1", host, -1, [[1]], 10)
    refused(UNSUPPORTED, "k=0", host, ref.GROUP, [[1]], 0)
    refused(UNSUPPORTED, "k=16385", host, ref.GROUP, [[1]], 16385)
    refused(INVALID, "nq=257", host, ref.GROUP, [[1]] * 257, 4)
    refused(INVALID, "nq=0", host, ref.GROUP, [], 4)
    refused(UNSUPPORTED, "request 1 has 257 triggers", host, ref.GROUP, [[1], [1] * 257], 4)
    ref.same(host(ref.GROUP, [[cases.T_ONE] * 256], 300), ref.recall(cases.ROWS, cases.ROW_OFFSET, *cases.table()[1], ref.GROUP,
                                                                     [[cases.T_ONE] * 256], 300))
    for bad in (np.nan, np.inf, -1.0, -5e-324):
        refused(INVALID, "trigger_value of trigger 1 of request 2", host, ref.TOPIC, [[1], [], [1, 2, 3]], 4, [[1.0], [], [1.0, bad, 1.0]])
    host(ref.GROUP, [[1], [], [1, 2, 3]], 4, [[1.0], [], [1.0, np.nan, 1.0]])                 # values are read in TOPIC mode only


def test_table_refusals():
    """what pg_hottable_upload refuses, through the same validation: each is PG_ERR_INVALID and names what it found"""
    what = {"row_outside": "item row 70000 .entry 0 of trigger 1. is outside", "nan_score": "entry 0 of trigger 0 is not finite",
            "inf_score": "entry 0 of trigger 1 is not finite", "pad_source": "source of entry 0 of trigger 0 is 0xFF",
            "unscored_with_score": "entry 1 of trigger 0 is marked unscored", "offsets_descend": r"offsets\[2\] is below offsets\[1\]",
            "list_too_long": "trigger 0 has 65537 entries"}
    bad = cases.bad_uploads()
    assert sorted(bad) == sorted(what)
    for name, tab in bad.items():
        refused(INVALID, what[name], host, ref.GROUP, [[0]], 4, tab=tab)
    # the same table without the defect, and a list of exactly 65536 with a row twice, are served
    ok = (np.array([0, 2, 3], np.uint64), np.array([1, 1, 3], np.uint32), np.array([1.0, 0.0, 2.0]), np.array([0, 0x80, 5], np.uint8))
    ref.same(host(ref.GROUP, [[1, 0]], 4, tab=ok), ref.recall(cases.ROWS, cases.ROW_OFFSET, *ok, ref.GROUP, [[1, 0]], 4))
    refused(INVALID, "rows=0", pa.hot_recall_host, 0, 0, *ok, ref.GROUP, [[0]], 4)
