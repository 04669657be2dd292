#!/bin/bash
# A/B variant of lib/libouro_verify.so that differs only in the latency-mode
# translation unit (kernels_lat.hip): the main build's other objects (the
# Makefile's kernel objects, HOSTOBJS and HOOKOBJS) are reused, kernels_lat.hip
# is compiled with the extra -D flags (the Makefile's LATOBJ / LATFLAGS).
#   tools/build_lat_variant.sh NAME [-DFLAG=VALUE ...]
set -euo pipefail
cd "$(dirname "$0")/../ouroboros-network_amd"
NAME=$1; shift
make -j8 LIBOUT="lib/variants/$NAME.so" LATOBJ="build/variant_$NAME/kernels_lat.o" \
  LATFLAGS="$*" "lib/variants/$NAME.so"
echo "lib/variants/$NAME.so"
