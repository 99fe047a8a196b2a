#!/bin/bash
# measurement aid: build kernel variants of libfastplong_amd.so side by side (gpurun_out/ab/<name>.so)
#   tools/ab_build.sh name "-DFPL_REDO_WAVES=4 ..." [source-dir]
# (the flags set numeric tunables.  An A/B of two implementations starts as a switch local to the working tree; when it is
#  decided, the losing side is deleted, not kept behind the switch)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; FLAGS=$2; SRC=${3:-$ROOT/fastplong_amd/csrc}
mkdir -p $ROOT/ab_libs
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -mllvm -amdgpu-atomic-optimizer-strategy=None $FLAGS \
    -I$ROOT/include -o $ROOT/ab_libs/$NAME.so $SRC/fpl_hip.hip 2>&1 | grep -E "error" || true
ls -la $ROOT/ab_libs/$NAME.so
