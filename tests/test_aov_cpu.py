"""CPU tests of the first-hit feature planes (mp_render_aov_device): the expectation model (tests/aov_model.py) against the
oracle's own tile render and against a scene computed by hand, the layered EXR writer, and header / ctypes mirror / library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, io
from tests import aov_model
from tests.aov_model import bits
from tests.conftest import TEAPOT

F = np.float32


# centre, silhouette, and a tile clipped by the frame's right / bottom edge (250x250 frame: the last tile is 26 wide)
@pytest.mark.parametrize("block", [(112, 112, 128, 128), (40, 96, 56, 112), (240, 120, 250, 136)])
@pytest.mark.parametrize("spp", [1, 10, 16])
def test_model_shade_equals_oracle_tile(oracle, teapot_oracle_bvh, block, spp):
    w = h = 250
    smp = oracle.build_sampler(oracle.teapot_camera(), w, h)
    ref, _ = teapot_oracle_bvh.render_tile(smp, w, h, spp, 7, *block)
    got = aov_model.planes(oracle, teapot_oracle_bvh.intersect, smp, w, spp, 7, block)
    assert np.array_equal(bits(got["shade"]), bits(ref))
    if block == (112, 112, 128, 128):
        assert ref[..., 3].min() > 0  # the centre tile really hits
    # alpha is the same number in both planes that carry it
    assert np.array_equal(bits(got["albedo"][..., 3]), bits(ref[..., 3]))


def test_model_shade_equals_oracle_sphere_tile(oracle):
    c, rad = (0.0, 1.5, 0.0), 1.25
    smp = oracle.build_sampler(oracle.teapot_camera(), 96, 96)
    block = (32, 24, 56, 48)
    ref, _ = oracle.render_tile_sphere(c, rad, smp, 96, 10, 3, *block)
    got = aov_model.planes(oracle, lambda r: oracle.sphere_intersect(c, rad, r), smp, 96, 10, 3, block)
    assert np.array_equal(bits(got["shade"]), bits(ref))
    assert 0 < ref[..., 3].sum() < ref[..., 3].size  # hits and misses


def test_model_on_a_hand_made_quad(oracle):
    """One flat quad in the plane y = 0 (normal +y), split into two triangles with materials 0 (a checker) and 1, seen straight
    down from y = 3 through a pinhole: normal (0, 1, 0) exactly, t = 3 / d.y, ids and the checker's cell as computed by hand."""
    pos = np.array([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2]], F)
    nrm = np.tile(np.array([0, 1, 0], F), (4, 1))
    tex = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    tri = np.array([[0, 2, 1], [0, 3, 2]], np.uint32)
    mat = np.array([0, 1], np.uint32)
    bvh = oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat)
    table = [{"albedo": (0.9, 0.8, 0.7), "albedo2": (0.1, 0.2, 0.3), "checker": 4.0}, ((0.25, 0.5, 0.75), 0.0)]
    bvh.set_materials(table, 1.0)
    cam = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(cam))
    oracle.lib().mpo_camera_look_at(C.byref(cam), oracle.vec3(0, 3, 0), oracle.vec3(0, 0, 0), oracle.vec3(0, 0, -1))
    cam.f_number = float("inf")  # pinhole: every ray starts at the eye
    res, spp = 24, 4
    smp = oracle.build_sampler(cam, res, res)
    got = aov_model.planes(oracle, bvh.intersect, smp, res, spp, 11, (0, 0, res, res), table)
    hit = got["ids"][..., 3] == 1
    full = got["shade"][..., 3] == 1.0  # every sample of the pixel hits
    assert hit.any() and full.any()
    n = got["normal"][full]
    assert np.all(n[:, 0] == 0) and np.all(n[:, 1] == 1) and np.all(n[:, 2] == 0)  # 4 x (0, 1, 0) / 4, exact
    # shade = |d . n| = |d.y| and t = 3 / |d.y| per sample: t * c = 3 for every sample, so the means obey
    # mean(t) * mean(c) >= 3 (Cauchy-Schwarz), and t >= 3
    t, c = got["normal"][full][:, 3].astype(np.float64), got["shade"][full][:, 0].astype(np.float64)
    assert np.all(t >= 3.0 - 1e-5) and np.all(t < 3.0 * 1.6) and np.all(t * c >= 3.0 * (1 - 1e-5)) and np.all(c <= 1.0)
    ids = got["ids"]
    assert set(np.unique(ids[hit][:, 0])) <= {0, 1} and np.all(ids[hit][:, 1] == 0)
    assert np.array_equal(ids[hit][:, 2], np.asarray(mat)[ids[hit][:, 0]])  # material of the triangle hit
    assert np.all(ids[~hit] == np.array([aov_model.NO_PRIM, 0, 0, 0], np.uint32))
    # albedo by hand, per sample, in float64: material 1 is plain; material 0 is a 4 x 4 checker over the quad's (u, v) = (x, z) / 4 + 0.5
    L = oracle.lib()
    for (y, x) in [tuple(p) for p in np.argwhere(full)[:: max(1, int(full.sum()) // 40)]]:
        acc = np.zeros(3, F)
        for s in range(spp):
            r = oracle.sample_ray(smp, int(x), int(y), L.mpo_sample_key(C.c_uint64(11), res, spp, int(x), int(y), s))
            k = -r.o[1] / r.d[1]
            px, pz = r.o[0] + k * r.d[0], r.o[2] + k * r.d[2]
            h = bvh.intersect(r)
            if h.material == 1:
                a = (0.25, 0.5, 0.75)
            else:
                u, v = (px + 2) / 4, (pz + 2) / 4
                fu, fv = u * 4, v * 4
                if min(abs(fu - round(fu)), abs(fv - round(fv))) < 1e-3:
                    a = None  # on a cell border: float32 and float64 may disagree
                    break
                a = (0.1, 0.2, 0.3) if (int(np.floor(fu)) + int(np.floor(fv))) % 2 else (0.9, 0.8, 0.7)
            acc = (acc + np.array(a, F)).astype(F)
        if a is not None:
            assert np.array_equal(bits(got["albedo"][y, x, :3]), bits((acc * (F(1) / F(spp))).astype(F))), (x, y)
    assert len(np.unique(bits(got["albedo"][full][:, 0]))) >= 3  # both checker colours and the plain material occur


def test_exr_layers_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    h, w = 7, 13
    nxyz = rng.standard_normal((h, w, 3)).astype(F)
    t = rng.random((h, w)).astype(F)
    rgb = rng.random((h, w, 3)).astype(F)
    alpha = rng.random((h, w)).astype(F)
    t[0, 0], alpha[1, 1] = np.inf, F(np.float32(1e-45))  # an infinity and a denormal survive
    nxyz.view(np.uint32)[2, 2, 0] = 0x7FC00123  # and a NaN payload
    p = str(tmp_path / "layers.exr")
    io.save_exr_layers(p, {"N": nxyz, "Z": t, "albedo": rgb, "A": alpha})
    names, got = io.load_exr_f32(p, layers=True)
    assert names == ["A", "N.X", "N.Y", "N.Z", "Z", "albedo.B", "albedo.G", "albedo.R"]
    assert names == sorted(names, key=lambda n: n.encode())
    for k, c in enumerate("XYZ"):
        assert np.array_equal(bits(got[f"N.{c}"]), bits(nxyz[:, :, k]))
    for k, c in enumerate("RGB"):
        assert np.array_equal(bits(got[f"albedo.{c}"]), bits(rgb[:, :, k]))
    assert np.array_equal(bits(got["Z"]), bits(t)) and np.array_equal(bits(got["A"]), bits(alpha))
    with pytest.raises(ValueError):
        io.save_exr_layers(p, {"Z": t, "A": alpha[:3]})
    with pytest.raises(ValueError):
        io.save_exr_layers(p, {"Z": t.astype(np.float64)})
    # save_exr is unchanged and the plain reader still returns R, G, B, A
    rgba = rng.random((h, w, 4)).astype(F)
    io.save_exr(p, rgba)
    assert np.array_equal(bits(io.load_exr_f32(p)), bits(rgba))
    assert io.load_exr_f32(p, layers=True)[0] == ["A", "B", "G", "R"]


def test_header_mirror_and_library_agree(tmp_path):
    L = _lib.lib()
    fn = L.mp_render_aov_device  # exported
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[6] is C.POINTER(_lib.AovPlanes) and fn.argtypes[7] is C.POINTER(_lib.LaunchExtras)
    assert mp.AovPlanes is _lib.AovPlanes
    src = tmp_path / "aov.c"
    fields = [f for f, _ in _lib.AovPlanes._fields_]
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "minipath_hip.h"', "int main(void) {",
         'printf("size %zu\\n", sizeof(mp_aov_planes));']
        + [f'printf("{f} %zu\\n", offsetof(mp_aov_planes, {f}));' for f in fields]
        + ["int (*fp)(mp_ctx*, const mp_scene*, const mp_camera_sampler*, const mp_settings*, const mp_block*, size_t, const mp_aov_planes*,"
           " const mp_launch_extras*, void*) = mp_render_aov_device; (void)fp;", "return 0;", "}"]))
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    so_dir = os.path.dirname(_lib.SO_PATH)
    subprocess.run(["gcc", "-std=c11", "-I", inc, "-c", str(src), "-o", str(tmp_path / "aov.o")], check=True)  # the prototype is as stated
    exe = tmp_path / "aov_layout"
    src2 = tmp_path / "aov2.c"
    src2.write_text(src.read_text().replace("int (*fp)", "/* int (*fp)").replace("(void)fp;", "*/"))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src2), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if l.strip())
    assert int(got["size"]) == C.sizeof(_lib.AovPlanes) == 32
    for f in fields:
        assert int(got[f]) == getattr(_lib.AovPlanes, f).offset
    assert fields == ["d_shade", "d_normal", "d_albedo", "d_ids"]
    assert os.path.isdir(so_dir)


def test_null_arguments_are_invalid_without_a_device():
    """The MP_ERR_UNSUPPORTED refusals need a context, hence a device (tests/test_gpu_aov.py); what can be reached without one is
    the NULL-argument check."""
    L = _lib.lib()
    host = mp.TriangleBvh.with_obj(TEAPOT)
    planes = _lib.AovPlanes()
    st = mp.RenderSettings(16, 1, (16, 16)).as_struct()
    smp = mp.Camera.teapot_view().build_sampler((16, 16)).as_struct()
    assert L.mp_render_aov_device(None, host.handle, C.byref(smp), C.byref(st), None, 0, C.byref(planes), None, None) == 1  # MP_ERR_INVALID
    assert L.mp_render_aov_device(None, None, None, None, None, 0, None, None, None) == 1
    assert L.mp_last_error()


def test_frame_renderer_has_the_aov_methods():
    assert callable(mp.FrameRenderer.render_aov) and callable(mp.FrameRenderer.untile_plane)
