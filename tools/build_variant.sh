#!/bin/bash
# tools/build_variant.sh <name> <source.hip> "<extra flags>": build/<name>/libdau_conv_hip.so = the TUNING build (-DDAU_TUNING:
# environment knobs readable) with one source recompiled under extra flags, by the Makefile's own rules (timing experiments;
# A/B against other libraries with tools/ab_multi.sh)
set -e
make -s -j8 -C "$(dirname "$0")/../dau-convnet_amd/csrc" variant NAME="$1" SRC="$2" FLAGS="$3"
echo built build/$1
