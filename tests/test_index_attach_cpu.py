"""CPU tests of serving through an attached index (pg_index_attach / _detach / _serving_stats): the three calls
are declared and exported and refuse NULLs, the ctypes mirror of pg_index_serving_stats_t has the header's layout (a C probe
built with the host compiler), and pa.Index has the new methods.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import pairec_amd as pa
from pairec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pairec_gpu.h")
PG_ERR_INVALID = -1
NAMES = ("pg_index_attach", "pg_index_detach", "pg_index_serving_stats")


def test_attach_calls_declared_and_exported():
    src = open(HEADER).read()
    for name in NAMES:
        assert "int %s(" % name in src, name
        assert name in _lib.EXPORTS
    assert "pg_index_serving_stats_t" in src
    L = _lib.load()
    for name in NAMES:
        assert hasattr(L, name)
    assert L.pg_index_attach(None, None) == PG_ERR_INVALID
    assert b"NULL" in L.pg_last_error()
    assert L.pg_index_detach(None, None) == PG_ERR_INVALID
    st = _lib.PgIndexServingStats()
    assert L.pg_index_serving_stats(None, C.byref(st)) == PG_ERR_INVALID
    assert L.pg_index_serving_stats(None, None) == PG_ERR_INVALID


def test_serving_stats_layout_matches_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler to build the layout probe")
    fields = [name for name, _ in _lib.PgIndexServingStats._fields_]
    probe = tmp_path / "probe.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pairec_gpu.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(pg_index_serving_stats_t));']
    lines += ['    printf("%%zu\\n", offsetof(pg_index_serving_stats_t, %s));' % f for f in fields]
    lines += ["    return 0;", "}"]
    probe.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.dirname(HEADER), str(probe), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(_lib.PgIndexServingStats)
    assert out[1:] == [getattr(_lib.PgIndexServingStats, f).offset for f in fields]
    # every counter of the issue's struct, in its order
    assert fields == ["plans", "plans_held", "queries_held", "replan_dense", "replan_rounds", "replan_overflow",
                      "replan_nonfinite", "skipped_stale", "skipped_switch"]


def test_index_class_has_serving_methods():
    for m in ("attach", "detach", "serving_stats"):
        assert callable(getattr(pa.Index, m, None)), m
