"""CPU test of TrafficControlSort's host side under sanitizers: tests/traffic_host_san.cpp, a program of its own with its own main, is
compiled together with the host code under test — csrc/traffic.hip (and csrc/traffic_host.hpp with it), host side instrumented with
ASan + UBSan where the compiler supports them — linked against the built library for everything else, and run: pg_traffic_compile /
pg_traffic_free, pg_traffic_table and pg_traffic_sort_host on hostile values and on a few hundred random configs.  The test passes
only on a clean exit.  Nothing sanitised is loaded into Python; no GPU is needed or touched."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pairec_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run(cmd, **kw):
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert out.returncode == 0, " ".join(cmd) + "\n" + out.stdout[-4000:]
    return out.stdout


def test_traffic_host_statement_under_asan_and_ubsan(tmp_path):
    lib_dir = os.path.join(ROOT, "pairec_amd")
    assert os.path.exists(os.path.join(lib_dir, "libpairec_gpu.so")), "build the library first"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run([HIPCC, "-x", "c++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        san = []                                                             # (a compiler without the runtimes: the run still checks the answers)
    host_san = [x for f in san for x in ("-Xarch_host", f)]
    objs = [str(tmp_path / "traffic.o"), str(tmp_path / "main.o")]
    _run([HIPCC, "-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-result", "-Wno-unused-value"] +
         host_san + ["-x", "hip", "-c", os.path.join(CSRC, "traffic.hip"), "-o", objs[0]])
    _run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-c", os.path.join(HERE, "traffic_host_san.cpp"), "-o", objs[1]])
    exe = str(tmp_path / "traffic_host_san")
    _run([HIPCC, "--offload-arch=gfx950"] + san[:1] + objs + ["-o", exe, "-L" + lib_dir, "-lpairec_gpu", "-Wl,-rpath," + lib_dir])
    # (the HIP runtime the library links keeps its own allocations until the process ends: leaks are not what this run looks for)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = _run([exe], env=env)
    assert "traffic_host_san OK" in out
