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


def _device_sources():
    """every source of the library with device code but mask_cache.h and the two headers below it (camera_rays.h, ray_math.h): the
    translation units (kernels*.hip) and the device headers they share"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")) and f not in ("mask_cache.h", "camera_rays.h", "ray_math.h", "mask_probe.hip", "probe.hip"):
            text = open(os.path.join(CSRC, f)).read()
            if "__device__" in text or "__global__" in text:
                out[f] = text
    return out


def test_kernels_take_predicates_from_header():
    sources = _device_sources()
    assert {"kernels.hip", "kernels_tiles.hip", "kernels_aov.hip", "kernels_paths.hip", "kernels_staged.hip", "kernels_queries.hip",
            "group_walk.h", "wave_common.h", "render_state.h", "packet_walk.h", "path_shading.h", "prof_counters.h"} <= set(sources)
    header = open(os.path.join(CSRC, "mask_cache.h")).read()
    probe = open(os.path.join(CSRC, "mask_probe.hip")).read()
    assert '#include "mask_cache.h"' in sources["wave_common.h"]
    assert '#include "mask_cache.h"' in probe
    for name in PREDICATES + HELPERS:
        assert _defines(header, name), f"mask_cache.h does not define {name}"
        for f, text in sources.items():
            assert not _defines(text, name), f"{f} defines {name} itself"
        assert not _defines(probe, name), f"mask_probe.hip defines {name} itself"
    # a source that uses a predicate or a helper has the header in its includes, directly or through the library's own headers
    def includes(f, seen):
        for h in re.findall(r'#include "(\w+\.h)"', open(os.path.join(CSRC, f)).read()):
            if h not in seen:
                seen.add(h)
                includes(h, seen)
        return seen
    for f, text in sources.items():
        if any(re.search(r"\b" + re.escape(n.replace("struct ", "")) + r"\b", text) for n in PREDICATES + HELPERS):
            assert "mask_cache.h" in includes(f, set()), f"{f} uses the mask cache's code without its header"
    # every unit that launches a cached row (MCACHE = true: `..., true>` in its sub-table of kernel_table.h) reaches the header
    table = open(os.path.join(CSRC, "kernel_table.h")).read()
    cached = {"MP_KERNELS_TILES": "kernels_tiles.hip", "MP_KERNELS_AOV": "kernels_aov.hip", "MP_KERNELS_PATHS": "kernels_paths.hip"}
    for sub in re.findall(r"#define (MP_KERNELS_\w+)\(X\)", table):
        rows = re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*\n)" % sub, table).group(1)
        # MCACHE is the fifth argument of the packet and feature-plane kernels and the fourth of the path kernel; nothing else has one
        has_cached = re.search(r"\b(render_tiles_packet_kernel|render_aov_packet_kernel)<([^,>]+,){4} true>|\brender_paths_kernel<([^,>]+,){3} true>", rows)
        assert (has_cached is not None) == (sub in cached), f"{sub}: the sub-tables with cached rows are {sorted(cached)}"
    for sub, unit in cached.items():
        assert "MP_FAMILY_LAUNCHER(%s)" % sub in sources[unit]
        assert {"mask_cache.h", "packet_walk.h"} <= includes(unit, set()), f"{unit} launches cached rows without the mask cache's header"
    # the walk uses them
    walk = [f for f, text in sources.items() if re.search(r"\bbool trace_packet_cached\(", text)]
    assert walk == ["packet_walk.h"], walk
    for name in ["mask_cache_ray_ok(", "mask_cache_begin_pass(", "bounds_may_hit<OCT>(", "tri_may_hit(", "slab<"]:
        assert name in sources[walk[0]], f"{walk[0]} no longer calls {name}"
