"""CPU test of the request coalescer's batching policy (pairec_amd/csrc/coalescer_policy.hpp): coalescer_policy_check.cpp, a program
of its own that includes nothing but that header, is built with the host compiler and run on hand-made time points.  It checks,
against values written out from the rules themselves: the inter-arrival EWMA from a first arrival (0, 100, 125, the clamp at
1e5 us, a negative gap); that a lone caller with a large EWMA goes at once and one with a small EWMA waits max_wait_us; that a
full recall queue is ready while the device is busy, a partial one only when idle, a partial rank or DPP queue at its deadline
while busy; that among ready queues the oldest head wins; that the wake time is the earliest eligible deadline, and a signal when
no slot is free; the rejoin hold (at once at the target, not before the window of 50 + us_per_caller * n closes otherwise), its
score for no, half and full return of the callers, and its re-arming at the sixteenth completion exactly while the score is
below one half; the three "full" rules and dpp_batch_limit at their edges.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "coalescer_policy OK" in out.stdout


def test_coalescer_policy_rules(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "coalescer_policy_check.cpp")]
    exe = tmp_path / "coalescer_policy_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe)
    # once more as a stand-alone binary under the address and undefined-behaviour sanitizers, where the compiler has their runtimes
    san = tmp_path / "coalescer_policy_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san)
