"""CPU test of the scratch arena's carving helper (pairec_amd/csrc/scratch_layout.hpp): scratch_layout_check.cpp, a program of
its own that includes nothing but the helper, is built with the host compiler and run.  It checks that a layout's measured
total is the end of its last region, that every region honours its alignment (64 and 256 bytes, packed neighbours), that regions
neither overlap nor leave declaration order, that a region of zero elements costs nothing and moves nobody, and that a layout
measured and then carved at a non-zero base gives base + offset.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def test_scratch_layout_helper(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the helper's check")
    exe = tmp_path / "scratch_layout_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "scratch_layout_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "scratch_layout OK" in out.stdout
