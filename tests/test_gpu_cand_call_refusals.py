"""GPU twin of tests/test_cand_call_refusals_cpu.py for the device entries — pg_candidates_trim_dev, pg_candidates_trim2_dev,
pg_candidates_blend_dev, pg_item_state_filter_dev, pg_candidates_classcut_dev: the same single faults (tests/cand_call_cases.py),
each refused before anything is launched, with the return code and the exact pg_last_error text recorded in
tests/golden/cand_call_refusals.json ("dev").  The trim and the blend never asked whether an output shares memory with its input:
those calls must still be accepted.  Every address is a zeroed 1 MiB device allocation, larger than any array of any call of the
table, so a call that is accepted — the valid one, the aliased ones — runs over empty requests.

`python tests/test_gpu_cand_call_refusals.py OUT.json` writes what the library as built answers, as the "dev" section of OUT.json."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cand_call_cases as cases                                   # noqa: E402
import pairec_amd as pa                                           # noqa: E402
from pairec_amd import _lib                                       # noqa: E402
from pairec_amd.engine import _blend_conf, _trim_rules            # noqa: E402

pytestmark = pytest.mark.gpu
BUF = 1 << 20
ENTRIES = ["pg_candidates_trim_dev", "pg_candidates_trim2_dev", "pg_candidates_blend_dev", "pg_item_state_filter_dev",
           "pg_candidates_classcut_dev"]
ALIAS_ACCEPTED = ["pg_candidates_trim_dev", "pg_candidates_blend_dev"]


class World:
    def __init__(self, ctx):
        self.ctx, self.L, self.bufs = ctx, _lib.load(), {}
        self.rules = _trim_rules([(0, pa.TRIM_FIX, 2), (1, pa.TRIM_ACCUMULATE, 3)])
        self.conf = _blend_conf((pa.BLEND_SNAKE_REFILL, 4, [(0, 1), (1, 1)]))
        self.fs = pa.Features(ctx, 16)
        self.fs.set_column("c0", pa.F_I32, np.arange(16, dtype=np.int32))
        self.cond = pa.Cond([{"Conditions": [{"Name": "c0", "Operator": "greater", "Type": "int", "Value": 3}]}], [("c0", pa.F_I32)])
        self.cc = pa.Classcut([("recall_score > 0.5", pa.TRIM_FIX, 2), ("recall_score <= 0.5", pa.TRIM_ACCUMULATE, 3)])

    def mem(self, name):
        if name not in self.bufs:
            self.bufs[name] = self.ctx.to_device(np.zeros(BUF, np.uint8))
        return self.bufs[name]

    def close(self):
        self.ctx.synchronize()
        for p in self.bufs.values():
            self.ctx.free(p)
        self.cond.free()
        self.cc.free()
        self.fs.destroy()

    def entry(self, name):
        """→ (the valid call's arguments, the entry's own required pointers, the call)"""
        L, a = self.L, cases.base_call(self.mem)
        a["ctx"] = self.ctx.h
        la = cases.list_args
        if name in ("pg_candidates_trim_dev", "pg_candidates_trim2_dev"):
            a["rules"] = self.rules
            return a, ["ctx", "rules"], lambda a: getattr(L, name)(a["ctx"], a["rules"], 2, a["nq"], a["cap"], *la(a))
        if name == "pg_candidates_blend_dev":
            a["conf"] = C.pointer(self.conf)
            return a, ["ctx", "conf"], lambda a: L.pg_candidates_blend_dev(a["ctx"], a["conf"], a["nq"], a["cap"], *la(a))
        if name == "pg_item_state_filter_dev":
            a.update(c=self.cond.h, fs=self.fs.h)
            return a, ["ctx", "c", "fs"], lambda a: L.pg_item_state_filter_dev(a["ctx"], a["c"], a["fs"], a["nq"], a["cap"], *la(a)[:9], None, None,
                                                                               *la(a)[9:])
        a["c"] = self.cc.h
        return a, ["ctx", "c"], lambda a: L.pg_candidates_classcut_dev(a["ctx"], a["c"], None, a["nq"], a["cap"], *la(a))

    def answers(self):
        """{entry: {fault: [code, text]}}, the valid call ("none") first; the stream is drained after every accepted call"""
        out = {}
        for name in ENTRIES:
            a, lead, call = self.entry(name)
            for fault, changes in [("none", [])] + cases.list_faults(lead):
                rc = call(cases.apply(a, changes))
                out.setdefault(name, {})[fault] = [rc, self.L.pg_last_error().decode("utf-8", "replace") if rc else ""]
                if rc == 0:
                    self.ctx.synchronize()
        return out


@pytest.fixture(scope="module")
def answers(ctx):
    w = World(ctx)
    got = w.answers()
    w.close()
    return got


def test_dev_refusals_answer_as_recorded(answers):
    want = cases.golden("dev")
    for entry in ENTRIES:
        for fault, got in answers[entry].items():
            print(entry, fault, got)
            assert got == want[entry][fault], (entry, fault)
        assert sorted(answers[entry]) == sorted(want[entry]), entry


def test_only_the_filter_and_the_cuts_refuse_an_aliased_output(answers):
    for entry in ENTRIES:
        for i, _ in cases.OVERLAPS:
            got = answers[entry]["overlap_" + i]
            assert got == ([0, ""] if entry in ALIAS_ACCEPTED else [-1, entry + ": an output overlaps its input"]), (entry, i)
        for fault, (rc, text) in answers[entry].items():
            if fault != "none" and not fault.startswith("overlap_"):
                assert rc != 0 and text.startswith(entry + ": "), (entry, fault, text)
        assert answers[entry]["none"] == [0, ""]


def test_the_context_serves_after_the_refusals(ctx, answers):
    rows = np.arange(8, dtype=np.uint64).reshape(1, 8)
    score = np.arange(8, dtype=np.float64).reshape(1, 8)
    out = ctx.candidates_trim([(pa.TRIM_ANY, pa.TRIM_FIX, 3)], rows, score)
    assert out[0].tolist() == [[7, 6, 5]] and out[6].tolist() == [3]


if __name__ == "__main__":
    with pa.Context(0) as c:
        w = World(c)
        rec = w.answers()
        w.close()
    with open(sys.argv[1], "w") as f:
        json.dump({"dev": rec}, f, indent=1, sort_keys=True)
    print("recorded", sum(len(v) for v in rec.values()), "calls")
