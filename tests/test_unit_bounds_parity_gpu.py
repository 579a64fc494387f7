"""Frames through the mask cache's corner bounds (mask_cache_begin_unit) against the oracle, bit for bit: an interior view, the teapot
view, a pinhole and an f/0.7 lens at 16, 64 and 256 samples per pixel (units of 4 and of 16 samples in flight, 4 to 16 passes
each), with the cache on and off, and with the cache on in the two builds of the library with other margins
(minipath_amd/csrc/Makefile, `make test-variants`): none, and -1/4, under which the first pass of nearly every unit leaves the
bounds the unit adopted, so that widening and clearing after an adoption is what renders the frame.  (With no margin the corner
bounds still hold every ray counted -- they bound the lens disc by its square -- hence the negative one.)  The -1/4 build counts
its bound sets (MP_PROF_MISSES): the test asserts more than 1.5 per unit on a frame of the interior view, where the shipped
margin has 1.00 -- every unit adopts once, and a B of half the corners' extent cannot hold a pass of 64 rays spread over it.

Each build renders in a process of its own (tests/walk_frames.py, run_in_variant), which calls variant_frames."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests.conftest import TEAPOT
from tests.dispatch_cases import launched
from tests.walk_frames import Counters, assert_same_bits, counted, run_in_variant

pytestmark = pytest.mark.gpu

RES, TILE, SEED = (96, 64), 32, 0x5EED
SPPS = (16, 64, 256)
ATRIUM_DETAIL = 0.05
VIEWS = {  # name -> scene, eye, look-at, f-number (None: the teapot view's own camera)
    "atrium": ("atrium", (-16.0, 4.2, 0.8), (12.0, 5.5, -0.5), 4.0),
    "teapot": ("teapot", None, None, 4.8),
    "pinhole": ("teapot", None, None, 1e9),
    "f/0.7": ("atrium", (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0), 0.7),
}


def render_all(modes):
    """{f"{view}/{spp}/{mode}": image} with this process's library"""
    import torch

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
    lib = _lib.lib()
    if not counted(lib):
        return None
    prof = Counters(lib)
    c = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, ATRIUM_DETAIL), c))
    _, eye, at, fnum = VIEWS["atrium"]
    fr = mp.FrameRenderer(scene, mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(fnum), mp.RenderSettings(TILE, 64, RES, seed=SEED))
    prof.reset()
    fr.render()
    sets = prof.read()["bound_sets"]
    in_flight = int(launched(c)[0].split("<")[1].split(",")[0])  # S samples of a pixel per pass: a unit is 64 / S pixels
    return sets / (RES[0] * RES[1] * in_flight // 64)


def variant_frames():
    """what a variant's process renders: the cases with the cache on, and the bound sets per unit where the build counts"""
    frames = render_all((1,))
    sets = bound_sets_per_unit()
    if sets is not None:
        frames["bound_sets_per_unit"] = np.float64(sets)
    return frames


@pytest.fixture(scope="module")
def expected(oracle, teapot_oracle_bvh):
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
        assert_same_bits(img, expected[key.rsplit("/", 1)[0]], f"{what} {key} against the oracle")


def test_default_margin_cache_on_and_off(expected):
    compare(render_all((1, 0)), expected, "shipped margin, view/spp/cache")


@pytest.mark.parametrize("variant", ["margin0", "shrunk"])
def test_other_margins(expected, variant, tmp_path):
    got = run_in_variant(variant, "tests.test_unit_bounds_parity_gpu:variant_frames", tmp_path, timeout=900)
    sets = got.pop("bound_sets_per_unit", None)
    compare(got, expected, f"{variant}, view/spp/cache")
    if variant == "shrunk":
        print(f"shrunk: {float(sets):.3f} bound sets per unit")
        assert float(sets) > 1.5, "the -1/4 build does not widen after adopting"
