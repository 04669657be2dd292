#!/bin/bash
# Build an A/B variant of lib/libouro_verify.so with extra -D flags into
# lib/variants/NAME.so (tools/ab_variants.py, tools/ab_latency.py --libs).
# The units, their flags and the link are the Makefile's own (its B, LIBOUT
# and XFLAGS variables): a variant links every unit the product does.
#   tools/build_variant.sh NAME [-DFLAG=VALUE ...]
set -euo pipefail
cd "$(dirname "$0")/../ouroboros-network_amd"
NAME=$1; shift
make -j8 B="build/variant_$NAME" LIBOUT="lib/variants/$NAME.so" XFLAGS="$*" \
  "lib/variants/$NAME.so"
echo "lib/variants/$NAME.so"
