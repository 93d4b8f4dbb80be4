"""CPU test of what a table carries beside its rows (pairec_amd/csrc/table_state.hpp): table_state_check.cpp, a program of its own
that includes nothing but that header, is built with the host compiler and run.  It checks TableLearned's update rules against
values written out from the rules themselves — the running averages (seeded by the first sample: 100, 125, 143.75), the
record-area scale (0 -> 2 -> 4 -> 8 -> 16, refused at the maximum, never at a maximum of 1), the predictor's back-off (128 ... 4096,
with and without forgetting the observations), the later-snapshot rule, the change of K, the screen's overflow streak and its
64-batch back-off — that each of the three reset moments clears its own fields and no others, that std::swap exchanges every field
of both structs, and that TableDerived lists its nine owned allocations once.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "table_state OK" in out.stdout


def test_table_state_rules(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "table_state_check.cpp")]
    exe = tmp_path / "table_state_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe)
    # once more as a stand-alone binary under the address and undefined-behaviour sanitizers, where the compiler has their runtimes
    san = tmp_path / "table_state_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san)
