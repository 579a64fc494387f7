"""The cached packet walk's early-outs of a triangle test (minipath_amd/csrc/mask_cache.h: tri_exit1_key, tri_exit2_key) on the GPU,
through libmp_mask_probe.so: the probe compiles the helpers the walk inlines.  One wave per case: a triangle and 64 rays inside a
generated box (the aimed, near-miss, degenerate and planar modes of the tri_may_hit probe), some of them disabled; the wave leaves
the triangle at stage 1 or 2 when every lane is surely rejected.  No case that the wave leaves may have a live ray that the plain
per-ray sequence (`1.0f / det`) accepts; and the probe must have met hits, exits at either stage and exits that only the far-side
keys give, or it has proved nothing."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_mask_probe.so")
NCASES = 1 << 20


def test_wave_exits_against_per_ray_sequence():
    import torch

    # (the renderer's HIP runtime is initialised before the probe's copy loads, the order the whole suite has)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    torch.zeros(1, device="cuda")
    L = C.CDLL(SO)
    L.mp_mask_probe_exits.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    o = np.zeros(8, np.uint64)
    rc = L.mp_mask_probe_exits(0xE817, NCASES, o.ctypes.data)
    assert rc == 0, f"HIP error {rc}"
    print(f"tri exits: cases {o[1]}, violations {o[0]}, some live ray hits {o[3]}, left at stage 1 {o[4]}, at stage 2 only {o[5]}, "
          f"left by the far side alone {o[6]}")
    assert o[1] == NCASES
    assert o[0] == 0, f"{o[0]} cases left although a live ray hits; first case {o[2]}"
    assert o[3] > 0 and o[4] > 0 and o[5] > 0, "no hits, or no exits at one of the stages: the probe proves nothing"
    assert o[6] > 0, "no exit that needs the far-side keys"
