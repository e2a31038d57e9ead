#!/bin/bash
# Cross-compiled variants of libtwl_align.so for the geometry experiments (tools/exp_thr.py, tools/lone_pair_probe.py):
# The throughput-geometry switch is not in the product source: `git apply tools/exp/thr_geometry.patch` first (tools/exp/README.md).
# Nor are the switches of the diagonal step and of the latency geometry (-DTWL_EXP_NOPRIO, _QPRE, _SALU, _VALU, _PACKED_SCORE, -DTWL_TB_ALWAYS, -DTWL_EXP_LAT_W / _LAT_RPL):
# `git apply tools/exp/step_switches.patch` first; without the patch such a flag builds the product kernel unchanged.
#   bash tools/build_exp.sh <name> -DTWL_EXP_THR_W=4 -DTWL_EXP_THR_RPL=2 -DTWL_EXP_THR_MINW=5     ->  build_exp/<name>.so  (+ <name>.resources: registers, scratch, LDS per kernel)
set -e
cd "$(dirname "$0")/.."
mkdir -p build_exp
name=$1; shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -std=c++17 '-DTWL_SOURCE_HASH="experiment"' "$@" \
    -Rpass-analysis=kernel-resource-usage -o build_exp/$name.so twilight_amd/csrc/twl_align.hip 2> build_exp/$name.resources
grep -A12 "talco_lean_kernelILi6ELi${W:-4}" build_exp/$name.resources | head -0
