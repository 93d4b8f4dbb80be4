#!/bin/bash
# Builds the library's host code with ASan + UBSan (device code as usual) into pairec_amd/csrc/_build_san, links
# scripts/classcut_host_san.cpp — a stand-alone program with its own main — against it and runs it on the CPU: pg_classcut_compile,
# pg_classcut_out_cap, pg_classcut_masks_host and pg_candidates_classcut_host on a fixed table of well-formed cases and of malformed
# expressions (unterminated quotes, 10 000 nested parentheses, a 1 MB input, an empty string).  Nothing sanitised is loaded into
# Python; no GPU is needed or touched.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined"
make -C pairec_amd/csrc -j"${JOBS:-8}" -s BUILD=_build_san OUT=_build_san/libpairec_gpu_san.so \
     CXXFLAGS="-O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-result -Wno-unused-value $SAN"
$HIPCC -x c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/classcut_host_san.cpp \
       -o pairec_amd/csrc/_build_san/classcut_host_san -Lpairec_amd/csrc/_build_san -lpairec_gpu_san -Wl,-rpath,"$PWD/pairec_amd/csrc/_build_san"
# (the HIP runtime keeps its own allocations until the process ends: leaks are not what this run looks for)
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1 pairec_amd/csrc/_build_san/classcut_host_san
