"""The refusal table of the candidate-list entry points, shared by tests/test_cand_call_refusals_cpu.py (the host statements) and
tests/test_gpu_cand_call_refusals.py (the device entries): one valid call per entry point — every optional array given, two
planes in each set — and single faults applied to it.  What a call answers (its return code and pg_last_error text) was recorded
from the library before the entry points' shared checks were stated once (tests/golden/cand_call_refusals.json); a call must
still answer the same, and a call with two faults must still report the same one.

A call's list arguments are held by name, in the ABI's order (LIST), as addresses; `mem` gives the addresses: host arrays for
the host statements, device allocations for the device entries.  Nothing here reads or writes through them."""
import json
import os

NQ, CAP = 2, 8
LIST = ["rows", "score", "source", "count", "planes_f64", "n_f64", "source_mask", "planes_f32", "n_f32",
        "out_rows", "out_score", "out_source", "out_planes_f64", "out_source_mask", "out_planes_f32", "out_count"]
REQUIRED = ["rows", "score", "out_rows", "out_score", "out_count"]
PAIRS = [("source", "out_source"), ("planes_f64", "out_planes_f64"), ("source_mask", "out_source_mask"), ("planes_f32", "out_planes_f32")]
OVERLAPS = [("rows", "out_rows"), ("score", "out_score"), ("source", "out_source"), ("source_mask", "out_source_mask"),
            ("planes_f64", "out_planes_f64"), ("planes_f32", "out_planes_f32")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cand_call_refusals.json")


def base_call(mem):
    """the valid call: mem(name) → the address of a buffer large enough for any array of the call"""
    a = {k: mem(k) for k in LIST if not k.startswith("n_")}
    a.update(n_f64=2, n_f32=2, nq=NQ, cap=CAP)
    return a


def list_faults(lead=()):
    """(name, [(argument, value)]) of every single fault of a list call and the double faults that pin the order; lead: the entry's
    own leading pointers (its context, rules or compiled set), each required"""
    f = [("null_" + k, [(k, None)]) for k in list(lead) + REQUIRED]
    f += [("nq_0", [("nq", 0)]), ("nq_257", [("nq", 257)]), ("cap_0", [("cap", 0)]), ("cap_16385", [("cap", 16385)])]
    for i, o in PAIRS:
        f += [("no_" + o, [(o, None)]), ("no_" + i, [(i, None)])]
    for n in ("n_f64", "n_f32"):
        f += [(n + "_0", [(n, 0)]), (n + "_9", [(n, 9)])]
    f += [("overlap_" + i, [(o, "=" + i)]) for i, o in OVERLAPS]
    f += [("two_null_rows_nq_0", [("rows", None), ("nq", 0)]), ("two_cap_0_no_out_source", [("cap", 0), ("out_source", None)]),
          ("two_n_f64_9_overlap_rows", [("n_f64", 9), ("out_rows", "=rows")]), ("two_nq_257_no_planes_f32", [("nq", 257), ("planes_f32", None)])]
    return f


def apply(args, changes):
    a = dict(args)
    for k, v in changes:
        a[k] = a[v[1:]] if isinstance(v, str) and v.startswith("=") else v
    return a


def list_args(a):
    """the 16 list arguments of a call in the ABI's order"""
    return [a[k] for k in LIST]


def golden(section):
    with open(GOLDEN) as f:
        return json.load(f)[section]


def record(section, answers):
    """(maintenance) writes one section of the golden file: {entry: {fault: [code, text]}}"""
    data = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            data = json.load(f)
    data[section] = answers
    with open(GOLDEN, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
