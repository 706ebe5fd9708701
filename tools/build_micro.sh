#!/bin/bash
# Prebuild the micro-benchmarks and probes into tools/bin/ (git-ignored).  Cross-compiles for gfx950; nothing is run.
set -euo pipefail
cd "$(dirname "$0")" && mkdir -p bin
HIPCC=${HIPCC:-hipcc}
INC="-I../include -I../qagnn_amd/csrc"
# one kernel family each, the production sources compiled into the program
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -o bin/gather_micro gather_micro.hip
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 $INC -o bin/nn2_ablate nn2_ablate.hip
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 $INC -o bin/tn_ablate tn_ablate.hip
# placement probes (which blocks share a CU, which waves share a SIMD)
$HIPCC --offload-arch=gfx950 -O3 -o bin/cu_census cu_census.hip
$HIPCC --offload-arch=gfx950 -O3 -o bin/simd_probe simd_probe.hip
# whole-library variants for kernel A/B runs (QAGNN_LIB=tools/bin/libqagnn_hip_u6.so python bench.py ...): the library's own source list
# and flags, read from qagnn_amd/build.py
read -r -a FLAGS < <(python3 -c 'import sys; sys.path.insert(0, "../qagnn_amd"); import build; print(*build.FLAGS)')
read -r -a SRC < <(python3 -c 'import sys; sys.path.insert(0, "../qagnn_amd"); import build; print(*("../qagnn_amd/csrc/" + s for s in build.SOURCES))')
for u in 6 8; do $HIPCC "${FLAGS[@]}" -DEDGE_UNROLL=$u -o bin/libqagnn_hip_u$u.so "${SRC[@]}"; done
