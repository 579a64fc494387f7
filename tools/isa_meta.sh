#!/bin/bash
# Per-kernel register / spill / scratch metadata of gfx950 code objects (device-only compiles with the Makefile's flags, then the
# AMDGPU metadata notes).  usage: tools/isa_meta.sh [denoise|adaptive|temporal|secondary|resample|lights|sky] > profiles/rNN_isa_meta.txt
#   (no argument)  the code objects of libminipath_hip.so, one per translation unit (kernels*.hip), as one list sorted by kernel
#   denoise        ../denoise/atrous.hip, the code object of libminipath_denoise.so -> profiles/denoise/isa_meta.txt
#   adaptive       ../adaptive/adaptive.hip, the code object of libminipath_adaptive.so -> profiles/adaptive/isa_meta.txt
#   temporal       ../temporal/reproject.hip, the code object of libminipath_temporal.so -> profiles/temporal/isa_meta.txt
#   secondary      ../secondary/secondary.hip, the code object of libminipath_secondary.so -> profiles/secondary/isa_meta.txt
#   resample       ../resample/resample.hip, the code object of libminipath_resample.so -> profiles/resample/isa_meta.txt
#   lights         ../lights/lights.hip, the code object of libminipath_lights.so -> profiles/lights/isa_meta.txt
#   sky            ../sky/sky.hip, the code object of libminipath_sky.so -> profiles/sky/isa_meta.txt
set -e
cd "$(dirname "$0")/../minipath_amd/csrc"
if [ "$1" = denoise ]; then
  make -s ../denoise/atrous.gfx950.co
  COS=../denoise/atrous.gfx950.co
elif [ "$1" = adaptive ]; then
  make -s ../adaptive/adaptive.gfx950.co
  COS=../adaptive/adaptive.gfx950.co
elif [ "$1" = temporal ]; then
  make -s ../temporal/reproject.gfx950.co
  COS=../temporal/reproject.gfx950.co
elif [ "$1" = secondary ]; then
  make -s ../secondary/secondary.gfx950.co
  COS=../secondary/secondary.gfx950.co
elif [ "$1" = resample ]; then
  make -s ../resample/resample.gfx950.co
  COS=../resample/resample.gfx950.co
elif [ "$1" = lights ]; then
  make -s ../lights/lights.gfx950.co
  COS=../lights/lights.gfx950.co
elif [ "$1" = sky ]; then
  make -s ../sky/sky.gfx950.co
  COS=../sky/sky.gfx950.co
else
  make -s code-objects
  COS=$(echo kernels*.gfx950.co)
fi
for co in $COS; do /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$co"; done | python3 ../../tools/isa_meta.py
