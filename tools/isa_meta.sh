#!/bin/bash
# Per-kernel register / spill / scratch metadata of a gfx950 code object (device-only compile with the Makefile's flags, then the
# AMDGPU metadata note).  usage: tools/isa_meta.sh [denoise] > profiles/rNN_isa_meta.txt
#   (no argument)  kernels.hip, the code object of libminipath_hip.so
#   denoise        ../denoise/atrous.hip, the code object of libminipath_denoise.so -> profiles/denoise/isa_meta.txt
set -e
cd "$(dirname "$0")/../minipath_amd/csrc"
CO=kernels.gfx950.co
[ "$1" = denoise ] && CO=../denoise/atrous.gfx950.co
make -s "$CO"
/opt/rocm/lib/llvm/bin/llvm-readelf --notes "$CO" | python3 ../../tools/isa_meta.py
