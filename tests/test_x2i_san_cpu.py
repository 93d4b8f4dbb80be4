"""tests/x2i_check.cpp — the X table's upload validation on hostile CSR, the recall's argument checks and the U2I2X2I host statement
(on hand-worked tables and on the device tests' grid, whose answers are compared with tests/x2i_ref.py here), over csrc/x2i_host.hpp
alone — built with a host compiler and run as a stand-alone program: once plain and once more under the address and
undefined-behaviour sanitizers where the compiler has their runtimes.  Nothing sanitised is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import x2i_cases as cases
import x2i_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pairec_amd", "csrc")


def _run(exe, grid_dir, want):
    answers = grid_dir / "answers.bin"
    if answers.exists():
        answers.unlink()
    out = subprocess.run([str(exe), str(grid_dir)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "x2i OK" in out.stdout
    raw = answers.read_bytes()
    at = 0
    for name, (rows, scores, counts) in want.items():
        nq, k = rows.shape
        got_rows = np.frombuffer(raw, np.uint64, nq * k, at).reshape(nq, k)
        got_bits = np.frombuffer(raw, np.uint64, nq * k, at + nq * k * 8).reshape(nq, k)
        got_counts = np.frombuffer(raw, np.uint32, nq + 1, at + nq * k * 16)
        at += nq * k * 16 + (nq + 1) * 4
        assert got_counts[nq] == 0xFFFFFFFF, name                     # no request of the grid is beyond a limit
        assert np.array_equal(got_counts[:nq], counts), name
        assert np.array_equal(got_rows, rows), name
        assert np.array_equal(got_bits, np.ascontiguousarray(scores).view(np.uint64)), name
    assert at == len(raw)


def test_x2i_host_side(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    if cxx is None:
        pytest.skip("no host C++ compiler to build the header's check")
    built = cases.build()
    cases.write_grid(tmp_path, built)
    xl = ref.XLists(cases.ROWS, cases.N_X, cases.ROW_OFFSET)
    cases.upload(xl, built)
    want = {name: ref.x2i_recall(xl, trig, pref, k, normalize, max_rule) for name, (trig, pref, k, normalize, max_rule) in cases.grid().items()}
    build = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "x2i_check.cpp")]
    exe = tmp_path / "x2i_check"
    subprocess.check_call(build + ["-o", str(exe)])
    _run(exe, tmp_path, want)
    san = tmp_path / "x2i_check_san"
    if subprocess.call(build + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(san)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0:
        _run(san, tmp_path, want)
