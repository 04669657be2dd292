#!/bin/bash
# A/B variant of lib/libouro_verify.so that differs only in the latency-mode
# translation unit (kernels_lat.hip): the main build's other objects (the
# Makefile's kernels.o, HOSTOBJS and HOOKOBJS) are reused, kernels_lat.hip is
# compiled with the extra -D flags.
#   tools/build_lat_variant.sh NAME [-DFLAG=VALUE ...]
set -euo pipefail
cd "$(dirname "$0")/../ouroboros-network_amd"
NAME=$1; shift
B=build/variant_$NAME
mkdir -p "$B" lib/variants
OBJS="build/kernels.o build/pack.o build/host_path.o build/numa.o build/task_pool.o build/knobs.o build/byron_dlg.o build/api_batch.o build/raw_pipe.o build/multi.o build/runtime.o build/plan.o"
for o in $OBJS; do test -f "$o" || { echo "build the library first (make)"; exit 1; }; done
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function "$@" \
  -c -o "$B/kernels_lat.o" csrc/kernels_lat.hip
/opt/rocm/bin/hipcc --hip-link -shared -fPIC -o "lib/variants/$NAME.so" "$B/kernels_lat.o" $OBJS -lpthread
echo "lib/variants/$NAME.so"
