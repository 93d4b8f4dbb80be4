"""CPU test of what the candidate stages' host statements refuse — pg_candidates_trim2_host, pg_candidates_blend_host,
pg_candidates_classcut_host, pg_mix_sort_host — one fault per call (tests/cand_call_cases.py): each required pointer NULL, nq 0
and 257, cap 0 and 16 385, an optional array without its output and the reverse, 0 and 9 planes, each of the six overlaps where
the stage refuses overlap, and calls with two faults, which pin the order of the checks.  Every call must give the return code
and the exact pg_last_error text recorded in tests/golden/cand_call_refusals.json.  No GPU needed.

`python tests/test_cand_call_refusals_cpu.py` rewrites the "host" section of the golden file from the library as built."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cand_call_cases as cases                                   # noqa: E402
import pairec_amd as pa                                           # noqa: E402
from pairec_amd import _lib                                       # noqa: E402
from pairec_amd.engine import _blend_conf, _trim_rules            # noqa: E402

BUF = 1 << 20                                                     # (larger than any array of any call of the table)
_keep = {}


def mem(name):
    _keep.setdefault(name, np.zeros(BUF, np.uint8))
    return _keep[name].ctypes.data


def _objects():
    if "objects" not in _keep:
        _keep["objects"] = dict(
            rules=_trim_rules([(0, pa.TRIM_FIX, 2), (1, pa.TRIM_ACCUMULATE, 3)]),
            conf=_blend_conf((pa.BLEND_SNAKE_REFILL, 4, [(0, 1), (1, 1)])),
            c=pa.Classcut([("recall_score > 0.5", pa.TRIM_FIX, 2), ("recall_score <= 0.5", pa.TRIM_ACCUMULATE, 3)]),
            m=pa.Mix([{"MixStrategy": "fix_position", "Positions": [1], "Number": 1, "SourceMask": 1}], size=4),
            no_cols=(C.c_void_p * 1)())
    return _keep["objects"]


def _list_entry(name):
    L, o = _lib.load(), _objects()
    a = cases.base_call(mem)
    if name == "pg_candidates_trim2_host":
        a["rules"] = o["rules"]
        return a, ["rules"], lambda a: L.pg_candidates_trim2_host(a["rules"], 2, a["nq"], a["cap"], *cases.list_args(a))
    if name == "pg_candidates_blend_host":
        a["conf"] = C.pointer(o["conf"])
        return a, ["conf"], lambda a: L.pg_candidates_blend_host(a["conf"], a["nq"], a["cap"], *cases.list_args(a))
    a["c"] = o["c"].h
    return a, ["c"], lambda a: L.pg_candidates_classcut_host(a["c"], a["nq"], a["cap"], None, o["no_cols"], *cases.list_args(a))


def _mix_entry():
    L, o = _lib.load(), _objects()
    a = dict(m=o["m"].h, nq=cases.NQ, cap=cases.CAP, out_order=mem("out_order"), out_count=mem("out_count"))
    faults = [("null_" + k, [(k, None)]) for k in ("m", "out_order", "out_count")]
    faults += [("nq_0", [("nq", 0)]), ("nq_257", [("nq", 257)]), ("cap_0", [("cap", 0)]), ("cap_16385", [("cap", 16385)]),
               ("two_null_out_order_nq_0", [("out_order", None), ("nq", 0)]), ("two_nq_257_cap_0", [("nq", 257), ("cap", 0)])]
    return a, faults, lambda a: L.pg_mix_sort_host(a["m"], 0, a["nq"], a["cap"], None, o["no_cols"], mem("source"), None, mem("count"), None,
                                                   None, None, a["out_order"], a["out_count"])


LIST_ENTRIES = ["pg_candidates_trim2_host", "pg_candidates_blend_host", "pg_candidates_classcut_host"]


def table():
    """[(entry, fault, the call as a function of nothing → return code)], the valid call of every entry first (fault "none")"""
    t = []
    for name in LIST_ENTRIES:
        a, lead, call = _list_entry(name)
        for fault, changes in [("none", [])] + cases.list_faults(lead):
            t.append((name, fault, lambda a=a, changes=changes, call=call: call(cases.apply(a, changes))))
    a, faults, call = _mix_entry()
    for fault, changes in [("none", [])] + faults:
        t.append(("pg_mix_sort_host", fault, lambda a=a, changes=changes, call=call: call(cases.apply(a, changes))))
    return t


def answer(call):
    rc = call()
    return [rc, _lib.load().pg_last_error().decode("utf-8", "replace") if rc else ""]


def test_host_refusals_answer_as_recorded():
    want = cases.golden("host")
    seen = {}
    for entry, fault, call in table():
        got = answer(call)
        print(entry, fault, got)
        assert got == want[entry][fault], (entry, fault)
        seen.setdefault(entry, set()).add(fault)
    assert {e: sorted(f) for e, f in seen.items()} == {e: sorted(f) for e, f in want.items()}, "the table and the golden file list the same calls"


def test_the_table_refuses_what_it_should():
    """the golden file itself: the valid call passes and every fault is refused under the entry's name — but for an output that
    aliases its input, which only the V2 cut's host statement refuses (all six of them, in one text)"""
    want = cases.golden("host")
    for entry, faults in want.items():
        for fault, (rc, text) in faults.items():
            if fault == "none" or (fault.startswith("overlap_") and entry != "pg_candidates_trim2_host"):
                assert [rc, text] == [0, ""], (entry, fault)
            else:
                assert rc != 0 and text.startswith(entry + ": "), (entry, fault, text)
    for i, _ in cases.OVERLAPS:
        assert want["pg_candidates_trim2_host"]["overlap_" + i] == [-1, "pg_candidates_trim2_host: an output overlaps its input"]


if __name__ == "__main__":
    rec = {}
    for entry, fault, call in table():
        rec.setdefault(entry, {})[fault] = answer(call)
    cases.record("host", rec)
    print("recorded", sum(len(v) for v in rec.values()), "calls")
