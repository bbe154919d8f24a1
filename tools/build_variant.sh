#!/bin/bash
# A/B library variant: libmvs_amd_<name>.so built with extra flags
# (e.g. tools/build_variant.sh b2 -DMVS_BIN_PER=2; MVS_BIN_PER * 1024 must stay
# within k_bin's 4096 candidates per workgroup); run with MVS_LIB=... or
# VARIANTS=<name> tools/gpu_ab.sh.  Variants are scratch: delete them after.
# The sources are build_lib.SOURCES (one list).
set -euo pipefail
D=$(cd "$(dirname "$0")/.." && pwd)/simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd
N=$1; shift
SRC=$(python3 "$D/build_lib.py" --sources)
[ -n "$SRC" ]
cd "$D/csrc" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
  -mllvm -amdgpu-atomic-optimizer-strategy=None -ffp-contract=off -fno-fast-math -Wno-unused-function "$@" \
  -o "$D/libmvs_amd_$N.so" $SRC
