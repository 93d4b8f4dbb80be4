#!/bin/bash
# Builds the library's host code with ASan + UBSan (device code as usual) into pairec_amd/csrc/_build_san, links
# scripts/trim2_host_san.cpp — a stand-alone program with its own main — against it and runs it on the CPU: pg_trim2_out_cap and
# pg_candidates_trim2_host on the reference tests' inputs and a few hundred generated merges and rule lists.  Nothing sanitised is
# loaded into Python; no GPU is needed or touched.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined"
make -C pairec_amd/csrc -j"${JOBS:-8}" -s BUILD=_build_san OUT=_build_san/libpairec_gpu_san.so \
     CXXFLAGS="-O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-result -Wno-unused-value $SAN"
$HIPCC -x c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/trim2_host_san.cpp \
       -o pairec_amd/csrc/_build_san/trim2_host_san -Lpairec_amd/csrc/_build_san -lpairec_gpu_san -Wl,-rpath,"$PWD/pairec_amd/csrc/_build_san"
# (the HIP runtime keeps its own allocations until the process ends: leaks are not what this run looks for)
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1 pairec_amd/csrc/_build_san/trim2_host_san tests/golden/priority_adjust_count_v2.json
