"""CPU test of a rank model's host side (pairec_amd/csrc/rank_model.hpp): rank_model_check.cpp, a program of its own that
includes nothing of the project but that header, is built with the host compiler and run.  It checks the MFMA-fragment layout of
pack_weights (fp32, bf16, split bf16) and pack_weights_f16 (one and two products) element by element against index formulas and
round-to-nearest-even stated in the check itself, the fp16 modes' row scaling (zero row, both sides of a power of two, NaN, Inf,
factors outside fp32's normal range), every refusal of the blob parser with its status and exact text (lengths around each
header, one byte more and less, heads, widths, precision, kind, a non-finite weight, the two-tower header and an item-field
count whose product with k wraps in 32 bits), and for the smallest good blob of each kind every array offset and the upload list:
each destination once, the lo pointers at half.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "rank_model OK" in out.stdout


def test_rank_model_host_side(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "rank_model_check.cpp")]
    exe = tmp_path / "rank_model_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe)
    # once more as a stand-alone binary under the address and undefined-behaviour sanitizers, where the compiler has their runtimes
    san = tmp_path / "rank_model_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san)
