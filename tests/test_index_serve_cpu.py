"""CPU test of the exact IVF index's host-side rules (pairec_amd/csrc/index_serve.hpp): index_serve_check.cpp, a program of its
own that includes nothing but that header, is built with the host compiler — no ROCm include path — and run on hand-made values.
It checks, against values written out from the rules themselves: the five batch-size bands at their edges; that a band's switch
armed with 3 skips exactly three batches of that band and none of another, and that four threads take exactly 1,000 from a switch
armed with 1,000; a finished plan's verdict (non-finite over dense over rounds over overflow over held), which counters move,
that dense and rounds arm the band with index_skip_batches (0 arms nothing, 0xFFFFFFFF arms 0x7FFFFFFF) and that only a held plan
counts its pairs, live rows and longest scan; the fold of the serving counters into pg_index_stats; the pre-search verdict (stale,
then non-finite, then L2 at a dim other than 64 / 128); the refresh's choice of mode; the build's defaults and clamps; and the
filtered lists' cache: move-to-front on a hit, capacity 0, the trim to the calling context's capacity, key equality.  No GPU
needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "index_serve OK" in out.stdout


def test_index_serve_rules(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", CSRC, os.path.join(HERE, "index_serve_check.cpp")]
    exe = tmp_path / "index_serve_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe)
    # once more as a stand-alone binary under the address and undefined-behaviour sanitizers, where the compiler has their runtimes
    san = tmp_path / "index_serve_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san)
