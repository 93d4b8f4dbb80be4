"""CPU test of the recall plans' arithmetic (pairec_amd/csrc/recall_plan_math.hpp): recall_plan_math_check.cpp, a program of its
own that includes nothing but that header, is built with the host compiler and run.  It compares the header's functions — the
pilot sample's geometry (stride, sample blocks, K', whether the pilot plan is worth it, the coprime perm_mul), the Poisson seed
rank m0, k2 and the refinement's split point, the chunk schedule of the grow and safe plans and the sizes of the hit-record
areas — with the expressions the plans held inline before, restated literally, over rows in {0, 31, 32, 511, 4 096, 1 M, 100 M,
0xFFFFFFE0} x K in {1, 10, 200, 5 000, 16 384} x admitted rows in {all, a thousandth, none} x record scale in {1, 2, 16} x early
share in {512, 604} x growth in {2, 4, 8}, safe on and off, and stops at the first difference.  Properties: gcd(perm_mul, sample
blocks) = 1; a schedule's chunks tile [0, nb) and the loop ends; no safe chunk exceeds kCandSlack / 2 rows; cap_w >= floor_w; the
areas' byte size is 64-bit (19 327 352 832 bytes at K = 16 384 x 16).  Anchors for 256 CUs, six sigmas, a seed of 8 192 rows: 100 M
rows, K 5 000 -> stride 95, 32 894 sample blocks, K' 105, perm_mul 21 537, m0 13, k2 1 471; 1 M rows, K 200 -> 8, 3 906, 63, 187,
23, 101.  No GPU needed, nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "recall_plan_math OK" in out.stdout


def test_recall_plan_math(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "recall_plan_math_check.cpp")]
    exe = tmp_path / "recall_plan_math_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe)
    # once more as a stand-alone binary under the address and undefined-behaviour sanitizers, where the compiler has their runtimes
    san = tmp_path / "recall_plan_math_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san)
