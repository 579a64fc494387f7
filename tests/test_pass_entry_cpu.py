"""The one-test pass entry (mask_cache.h, mask_cache_pass_inside) is wired the way tests/test_pass_entry_gpu.py assumes: the probe
exports its entry point, the walk takes the decision from the header the probe compiles, behind its build switch, and the path
family switches it off for itself."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc")
SO = os.path.join(CSRC, "libmp_mask_probe.so")


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_probe_exports_the_entry_probe():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    nm = os.path.join("/opt/rocm/lib/llvm/bin", "llvm-nm")
    out = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", SO], capture_output=True, text=True, check=True).stdout
    assert "mp_mask_probe_entry" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_walk_takes_the_decision_from_the_header_behind_its_switch():
    header, walk, probe = read("mask_cache.h"), read("packet_walk.h"), read("mask_probe.hip")
    assert re.search(r"__device__[^;{(]*\bmask_cache_pass_inside\(", header)
    assert not re.search(r"__device__[^;{(]*\bmask_cache_pass_inside\(", walk + probe)
    assert "mask_cache_pass_inside(MaskCache{base}" in probe
    # one call in the walk, inside the switch's #ifndef block
    assert walk.count("mask_cache_pass_inside(mc, r, active)") == 1
    block = re.search(r"#ifndef MP_NO_ENTRY_FOLD\n(.*?)\n#else\n(.*?)\n#endif", walk, re.S)
    assert block and "mask_cache_pass_inside(mc, r, active)" in block.group(1) and "mask_cache_pass_inside" not in block.group(2)
    for route in block.groups():  # both routes keep the full guards
        assert "mask_cache_ray_ok(r)" in route and "mask_cache_begin_pass(mc, r, active, oct)" in route


def test_the_fold_keeps_a_nan():
    """the nine deviations are added, not folded with maxNum (which drops a NaN operand), and the test is !(sum == 0)"""
    body = re.search(r"uint32_t mask_cache_pass_inside\(.*?\n}\n", read("mask_cache.h"), re.S).group(0)
    assert "dev += bounds_deviation(" in body and "fmaxf" not in body
    assert "!(dev == 0.0f)" in body
    assert "(state & ~7u) == 0x100u" in body


def test_families():
    assert re.search(r"#ifndef MP_NO_ENTRY_FOLD\n#define MP_NO_ENTRY_FOLD\n#endif\n(.*\n)*#include \"packet_walk.h\"", read("kernels_paths.hip"))
    for unit in ("kernels_tiles.hip", "kernels_aov.hip"):
        assert "MP_NO_ENTRY_FOLD" not in read(unit), unit
