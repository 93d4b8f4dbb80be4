"""tests/hot_check.cpp — the list recall's host side over csrc/hot_host.hpp alone: the upload validation on hostile offsets and
entries, empty lists, n at its limits, the quota function on zero, tiny and huge values, and the host statement against a plain
restatement — built with a host compiler and run as a stand-alone program: once plain and once more under the address and
undefined-behaviour sanitizers where the compiler has their runtimes.  Nothing sanitised is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "hot OK" in out.stdout


def test_hot_host_side(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "hot_check.cpp")]
    exe = tmp_path / "hot_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe)
    san = tmp_path / "hot_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san)
