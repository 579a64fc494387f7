"""The mask-cache probe library exports its entry points, and the walk takes its predicates from mask_cache.h -- the header the probe
(tests/test_mask_cache_gpu.py) compiles -- so that the tested code stays the shipped code."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc")
SO = os.path.join(CSRC, "libmp_mask_probe.so")
ENTRY = ["mp_mask_probe_tri", "mp_mask_probe_box", "mp_mask_probe_ray_ok", "mp_mask_probe_dev", "mp_mask_probe_pass",
         "mp_mask_probe_dump", "mp_mask_probe_dump_dwords"]
PREDICATES = ["kCoordCap", "struct MaskCache", "wave_min3_max3", "mask_cache_ray_ok", "bounds_deviation", "mask_cache_begin_pass",
              "bounds_may_hit", "struct Iv", "iv_mul", "iv_fma", "tri_may_hit", "kMaskCacheDwords", "kHdrState", "hdr_lo"]
HELPERS = ["as_f", "as_u", "wave_lds_sync", "fms", "fma_dot", "slab", "struct Ray"]


def _defines(src, name):
    """does `src` define (not merely use) `name`?"""
    if name.startswith("struct "):
        return re.search(r"\b" + name + r"\s*\{", src) is not None
    return re.search(r"(__device__[^;{(]*|constexpr[^;{(=]*|#define\s+)\b" + re.escape(name) + r"\b\s*[(=\[<{]?", src) is not None


def test_probe_exports_entry_points():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    nm = os.path.join("/opt/rocm/lib/llvm/bin", "llvm-nm")
    cmd = [nm if os.path.exists(nm) else "nm", "-D", "--defined-only", SO]
    syms = set(line.split()[-1] for line in subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    missing = [e for e in ENTRY if e not in syms]
    assert not missing, f"libmp_mask_probe.so does not export {missing}"


def test_kernels_take_predicates_from_header():
    kernels = open(os.path.join(CSRC, "kernels.hip")).read()
    header = open(os.path.join(CSRC, "mask_cache.h")).read()
    probe = open(os.path.join(CSRC, "mask_probe.hip")).read()
    assert '#include "mask_cache.h"' in kernels and '#include "mask_cache.h"' in probe
    for name in PREDICATES + HELPERS:
        assert _defines(header, name), f"mask_cache.h does not define {name}"
        assert not _defines(kernels, name), f"kernels.hip defines {name} itself"
        assert not _defines(probe, name), f"mask_probe.hip defines {name} itself"
    # the walk uses them
    for name in ["mask_cache_ray_ok(", "mask_cache_begin_pass(", "bounds_may_hit<OCT>(", "tri_may_hit(", "slab<"]:
        assert name in kernels, f"kernels.hip no longer calls {name}"
