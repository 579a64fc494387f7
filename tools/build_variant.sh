#!/bin/bash
# usage: tools/build_variant.sh NAME "-DMACRO=..."  -- builds variants/libmp_NAME.so from the tree's sources with extra compile
# flags (A/B runs through tools/ab.sh / MINIPATH_HIP_SO) by the Makefile's variant rule, which knows the device flags: every
# translation unit with kernels is recompiled with the extra flags (MP_MCACHE_WPE, MP_PATHS_WPE, MP_PROF_NOWALK, MP_PROF_NOSHADE,
# ...), and the launch plans (launch_plan.cpp), which read the same macros as the kernels; the host objects are the normal build's.
set -e
cd "$(dirname "$0")/../minipath_amd/csrc"
make -s
rm -rf "variants/$1"  # (objects of an earlier build under this name, maybe with other flags)
make -s NAME="$1" FLAGS="$2" "../../variants/libmp_$1.so"
echo variants/libmp_$1.so
