#!/bin/bash
# Forward / dx time of the EXACT gather (--no-split) of one workload (DIAG_ARGS, default: the north-star shape) under diagnostic builds of k_gather_mfma.hip (their results are
# garbage, timing only): NOLDS = no tile reads, NOBARRIER = no per-channel barrier, DAU_GATHER_DEBUG=1 = no plane DMA.
# Run on the GPU box from the repo root (builds the variants with hipcc first).
set -e
cd "$(dirname "$0")/.."
for V in NOLDS NOBARRIER "NOLDS -DDAU_DIAG_NOBARRIER"; do
  tools/build_variant.sh diag_$(echo $V | tr -d ' -') k_gather_mfma.hip "-DDAU_DIAG_$V" >/dev/null 2>&1
done
mkdir -p build/diag_base; cp dau-convnet_amd/dau_conv/libdau_conv_hip_tuning.so build/diag_base/libdau_conv_hip.so
for L in build/diag_base build/diag_NOLDS build/diag_NOBARRIER build/diag_NOLDSDDAU_DIAG_NOBARRIER; do
  for D in 0 1; do
    DAU_CONV_LIB=$PWD/$L/libdau_conv_hip.so DAU_GATHER_DEBUG=$D timeout -k 10 300 python bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-layer --no-check --no-split $DIAG_ARGS 2>/dev/null | \
      python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$L debug=$D', d['roofline']['kernels']['gather_sum_fwd']['avg_ms'], d['roofline']['kernels']['gather_sum_dx']['avg_ms'])"
  done
done
