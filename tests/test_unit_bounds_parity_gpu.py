"""Frames through the mask cache's corner bounds (mask_cache_begin_unit) against the oracle, bit for bit: an interior view, the teapot
view, a pinhole and an f/0.7 lens at 16, 64 and 256 samples per pixel (units of 4 and of 16 samples in flight, 4 to 16 passes
each), with the cache on and off, and with the cache on in the two builds of the library with other margins
(minipath_amd/csrc/Makefile, `make test-variants`): none, and -1/4, under which the first pass of nearly every unit leaves the
bounds the unit adopted, so that widening and clearing after an adoption is what renders the frame.  (With no margin the corner
bounds still hold every ray counted -- they bound the lens disc by its square -- hence the negative one.)  The -1/4 build counts
its bound sets (MP_PROF_MISSES): the test asserts more than 1.5 per unit on a frame of the interior view, where the shipped
margin has 1.00 -- every unit adopts once, and a B of half the corners' extent cannot hold a pass of 64 rays spread over it.

Each build renders in a process of its own (MINIPATH_HIP_SO is read when the package loads); run as a program this file is that
process: it renders the cases and writes them to the .npz it is given."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES, TILE, SEED = (96, 64), 32, 0x5EED
SPPS = (16, 64, 256)
ATRIUM_DETAIL = 0.05
VIEWS = {  # name -> scene, eye, look-at, f-number (None: the teapot view's own camera)
    "atrium": ("atrium", (-16.0, 4.2, 0.8), (12.0, 5.5, -0.5), 4.0),
    "teapot": ("teapot", None, None, 4.8),
    "pinhole": ("teapot", None, None, 1e9),
    "f/0.7": ("atrium", (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0), 0.7),
}
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")


def render_all(modes):
    """{f"{view}/{spp}/{mode}": image} with this process's library"""
    import torch

    import minipath_amd as mp
    from minipath_amd import scenes
    from tests.dispatch_cases import launched

    out = {}
    for mode in modes:
        c = mp.Context(0)
        c.set_option("packet_mask_cache", mode)
        built = {"teapot": mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c)), "atrium": mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, ATRIUM_DETAIL), c))}
        for name, (scene, eye, at, fnum) in VIEWS.items():
            cam = mp.Camera.teapot_view() if eye is None else mp.Camera.default().look_at(eye, at, (0, 1, 0))
            for spp in SPPS:
                fr = mp.FrameRenderer(built[scene], cam.f_number(fnum), mp.RenderSettings(TILE, spp, RES, seed=SEED))
                fr.render()
                k = launched(c)
                assert len(k) == 1 and k[0].startswith("render_tiles_packet_kernel<") and k[0].endswith(", true>") == bool(mode), (name, spp, mode, k)
                img, _ = fr.untile()
                torch.cuda.synchronize()
                out[f"{name}/{spp}/{mode}"] = img.cpu().numpy()
    return out


def bound_sets_per_unit():
    """bound (re)sets per work unit of one frame of the interior view at 64 spp, in a build that counts them; None in others"""
    import torch

    import minipath_amd as mp
    from minipath_amd import _lib, scenes
    from tests.dispatch_cases import launched

    lib = _lib.lib()
    if not hasattr(lib, "mp_prof_read"):
        return None
    lib.mp_prof_read.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    c = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, ATRIUM_DETAIL), c))
    _, eye, at, fnum = VIEWS["atrium"]
    fr = mp.FrameRenderer(scene, mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(fnum), mp.RenderSettings(TILE, 64, RES, seed=SEED))
    out = (C.c_ulonglong * 4)()
    assert lib.mp_prof_read(out, 1) == 0
    fr.render()
    torch.cuda.synchronize()
    assert lib.mp_prof_read(out, 0) == 0
    in_flight = int(launched(c)[0].split("<")[1].split(",")[0])  # S samples of a pixel per pass: a unit is 64 / S pixels
    return out[3] / (RES[0] * RES[1] * in_flight // 64)


if __name__ == "__main__":
    frames = render_all((1,))
    sets = bound_sets_per_unit()
    if sets is not None:
        frames["bound_sets_per_unit"] = np.float64(sets)
    np.savez(sys.argv[1], **frames)
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(oracle, teapot_oracle_bvh):
    from minipath_amd import scenes

    orc = {"teapot": teapot_oracle_bvh, "atrium": oracle.Bvh.build(*scenes.atrium(1, ATRIUM_DETAIL))}
    exp = {}
    for name, (scene, eye, at, fnum) in VIEWS.items():
        if eye is None:
            oc = oracle.teapot_camera()
        else:
            oc = oracle.Camera()
            oracle.lib().mpo_camera_default(C.byref(oc))
            oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*eye), oracle.vec3(*at), oracle.vec3(0, 1, 0))
        oc.f_number = fnum
        for spp in SPPS:
            exp[f"{name}/{spp}"] = orc[scene].render_image_mt(oracle.build_sampler(oc, *RES), RES[0], RES[1], spp, SEED, TILE, 8)[0]
        assert np.count_nonzero(exp[f"{name}/{SPPS[0]}"][..., 3]) > 200, name  # the view does hit the scene
    return exp


def compare(got, expected, what):
    assert len(got) >= len(expected)
    for key, img in got.items():
        e = expected[key.rsplit("/", 1)[0]]
        diff = int(np.sum(np.ascontiguousarray(img).view(np.uint32) != np.ascontiguousarray(e).view(np.uint32)))
        assert diff == 0, f"{what} {key}: {diff} words differ from the oracle"


def test_default_margin_cache_on_and_off(expected):
    compare(render_all((1, 0)), expected, "shipped margin, view/spp/cache")


@pytest.mark.parametrize("variant", ["margin0", "shrunk"])
def test_other_margins(expected, variant, tmp_path):
    so = os.path.join(ROOT, "minipath_amd", "csrc", f"libminipath_hip_{variant}.so")
    if not os.path.exists(so):
        pytest.fail(f"{so} missing: run build() first")
    dst = str(tmp_path / "frames.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dst], env=dict(os.environ, MINIPATH_HIP_SO=so), cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    with np.load(dst) as z:
        compare({k: z[k] for k in z.files if k != "bound_sets_per_unit"}, expected, f"{variant}, view/spp/cache")
        if variant == "shrunk":
            print(f"shrunk: {float(z['bound_sets_per_unit']):.3f} bound sets per unit")
            assert float(z["bound_sets_per_unit"]) > 1.5, "the -1/4 build does not widen after adopting"
