"""GPU test (-m gpu): the host side gives back every device and pinned buffer it owns.  Contexts, scenes, groups, material
tables, worker slots, shards, gather and staging buffers are made and destroyed in cycles, and the device's used memory must
not grow by as much as the smallest of them."""
import gc

import numpy as np
import pytest

import minipath_amd as mp
from tests import meshes

pytestmark = pytest.mark.gpu
MIB = 1 << 20
RES, TS, BATCH = (1024, 1024), 32, 256
TABLES = ([(0.5, 0.0)], [{"albedo": (0.9, 0.4, 0.2), "emission": (0.0, 0.0, 0.1)}])


def _used():
    import torch

    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def _cycle(arrays, odd):
    ctxs = [mp.Context(0) for _ in range(2)]
    ctxs[0].set_option("render_batch_tiles", BATCH)
    inner, packets, shading, vn, vt, root, bmin, bmax = arrays
    members = [mp.TriangleBvh.from_arrays(inner, packets, shading, vn, vt, root, bmin, bmax, c) for c in ctxs]
    groups = [mp.ObjectGroup([m], [[0.0, 0.0, 0.0]]) for m in members]
    device_bytes = members[0].info().device_bytes
    for table in TABLES:
        for s in members + groups:
            s.set_materials(table, 0.8)
    cam = mp.Camera.default().look_at((0.0, 3.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    st = mp.RenderSettings(TS, 1, RES, seed=7)
    f, _ = mp.render_tile(mp.Scene(groups[1]), cam.build_sampler(RES), st, mp.ScreenBlock(480, 480, 512, 512))
    assert f[..., 3].max() == 1.0  # the tile shows the mesh
    done = []
    prog = mp.render(mp.Scene(groups[0]), cam, st, None, lambda b, p: done.append(p.finished))
    prog.wait()
    assert len(done) == (RES[0] // TS) * (RES[1] // TS)
    prog.close()
    mf = mp.MultiDeviceFrame([mp.Scene(m) for m in members], cam, st)
    for staged in (1, 0):
        ctxs[0].set_option("multi_gather_staged", staged)
        nxt, img, _ = mf.render_pass(0, 0)
        assert nxt == 1 and ctxs[0].query("multi_staged_ranks") == staged
    assert float(img[..., 3].max().item()) == 1.0
    del mf, img
    # odd cycles: the members' handles go first and the groups keep their arrays alive; even cycles: groups before members
    for s in (members + groups) if odd else (groups + members):
        s.close()
    for c in ctxs:
        c.close()
    return device_bytes


def test_cycles_of_contexts_and_scenes_do_not_grow_device_memory():
    """Five cycles of {two contexts, a scene and a group of it per context, set_materials twice, mp_render_tile, render() with
    callbacks, a staged and a direct gathered mp_render_pass_multi, everything destroyed} at 1 spp: used device memory after cycle 5
    exceeds that after cycle 2 by less than 4 MiB, which is less than any one of the tracked allocations (asserted below)."""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    host = mp.TriangleBvh.build(*meshes._grid(160, 3))
    i = host.info()
    arrays = host.export() + (i.root_link, tuple(i.bbox_min), tuple(i.bbox_max))
    host.close()
    tiles = (RES[0] // TS) * (RES[1] // TS)
    tile_bytes = TS * TS * 16
    assert tiles * tile_bytes >= 4 * MIB  # the gather buffer (16 MiB)
    assert tiles // 2 * tile_bytes >= 4 * MIB  # one rank's shard and its pinned stage (8 MiB)
    assert BATCH * tile_bytes >= 4 * MIB  # one worker slot's f32 buffer
    used = []
    for cycle in range(1, 6):
        assert _cycle(arrays, cycle % 2 == 1) >= 4 * MIB  # the scene's device arrays
        gc.collect()
        used.append(_used())
        print(f"cycle {cycle}: {used[-1] / MIB:.1f} MiB used")
    growth = used[4] - used[1]
    print(f"growth from cycle 2 to cycle 5: {growth / MIB:.2f} MiB")
    assert growth < 4 * MIB, [u / MIB for u in used]
