"""The cases of tests/camera_cases.py are what their names say, shown without a GPU: the builder-made samplers equal the oracle's bit
for bit; the floats have the property each case is named for; the scaled cases split the frame at the windows of rm::ray_dir; every
finite case's oracle frame holds hits and misses, the non-finite ones none and no NaN; a power-of-two film scale leaves the oracle's
frame unchanged while nothing underflows; the unit bounds model (tools/analytic_bounds.py) adopts or declines as the case intends;
the routes' kernel names are those the launch plans give; and a kernel that dropped lens_weight or sized a sensor_is_width camera
by its height would not pass: a numpy model with either mistake differs from the oracle's frame in hundreds of pixels."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from tests import aov_pass_model, camera_cases as cc, dispatch_cases as dc, plan_probe as pp, temporal_cases as tc, temporal_model as tm
from tests.camera_cases import F, INF
from tests.conftest import TEAPOT
from tests.test_unit_bounds_cpu import _model, check_invariants, shipped_margin

# hit pixels (alpha > 0) of the oracle's 16-spp frame, of 1536
HITS = {"inf_focus_open": 583, "near_focus": 1245, "focus_zero": 0, "wide": 345, "wide_pinhole": 346, "tele": 588, "portrait": 276,
        "rolled": 592, "look_direction": 585, "scaled_mixed": 346, "scaled_high": 346, "scaled_subnormal": 585, "scaled_flush": 0,
        "anisotropic": 310, "sheared": 554, "negative_lens": 587}
PINHOLE_HITS = 585
# pixel centres with a direction component below 2^-40 for wide_pinhole * 2^k, and with the sum of squares >= 2^80
BELOW_COMPONENT = {-34: 1536, -33: 1366, -32: 906, -31: 524, -30: 340}
SUM_ABOVE = {45: 16, 46: 1088, 47: 1536}
# 2 x 2 units of 384 whose corner bounds the model adopts
ADOPTED = {"inf_focus_open": 330, "near_focus": 0, "focus_zero": 0, "wide": 308, "wide_pinhole": 308, "tele": 330, "portrait": 322,
           "rolled": 331, "look_direction": 330, "scaled_mixed": 308, "scaled_high": 308, "scaled_subnormal": 330, "scaled_flush": 0,
           "anisotropic": 345, "sheared": 338, "negative_lens": 330}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_frames = {}


def oracle_frame(oracle, bvh, values, res, spp=16):
    """the oracle's frame of a sampler given as its 15 floats, cached"""
    values = np.ascontiguousarray(values, F)
    key = (values.tobytes(), res, spp)
    if key not in _frames:
        with np.errstate(all="ignore"):
            _frames[key] = bvh.render_image_mt(oracle.sampler_from_array(values), res[0], res[1], spp, cc.SEED, cc.TILE, 8)[0]
    return _frames[key]


def case_frame(oracle, bvh, name, spp=16):
    c = cc.cases()[name]
    return oracle_frame(oracle, bvh, c["values"], c["res"], spp)


def pixels_differing(a, b):
    return int((bits(a) != bits(b)).any(-1).sum())


# ---- the samplers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.BUILDERS) + list(cc.BASES))
def test_builder_samplers_equal_the_oracles(oracle, name):
    """mp.Camera(...).build_sampler == mpo_camera_build_sampler in all 15 floats for these focal lengths, sensors, placements and
    focus distances, 0 and inf included (test_camera_matches_oracle_bitwise, widened)"""
    spec = {**cc.BUILDERS, **cc.BASES}[name]
    res = spec.get("res", cc.RES)
    got = cc.product_camera(spec).build_sampler(res).as_array()
    want = oracle.build_sampler(cc.oracle_camera(oracle, spec), *res).as_array()
    assert got.dtype == F and got.size == 15
    assert np.array_equal(bits(got), bits(want)), (name, got, want)
    if name in cc.BUILDERS:
        c = cc.cases()[name]
        assert np.array_equal(bits(c["values"]), bits(want)) and np.array_equal(bits(c["sampler"].as_array()), bits(want))
        assert np.array_equal(bits(c["camera"].build_sampler(res).as_array()), bits(want))


def test_hand_made_samplers_travel_unchanged():
    """FixedSampler hands the product the very floats the oracle gets, subnormal film scales included, at any resolution"""
    for name in cc.HAND_MADE:
        c = cc.cases()[name]
        assert c["built"] is None
        for res in (c["res"], (1920, 1080)):
            smp = c["camera"].build_sampler(res)
            assert np.array_equal(bits(smp.as_array()), bits(c["values"])), name
            assert bytes(smp.as_struct()) == c["values"].tobytes() == bytes(c["sampler"]), name


def test_case_properties():
    """each case is what its name says, on the floats"""
    v = {n: c["values"] for n, c in cc.cases().items()}
    teapot, pinhole, wide_pinhole = (cc.base_values(n) for n in ("teapot", "pinhole", "wide_pinhole"))
    assert set(v) == set(cc.NAMES) and len(cc.NAMES) == 16
    assert v["inf_focus_open"][14] == 0 and v["inf_focus_open"][13] == F(50e-3) / (F(2) * F(1.4)) > 0
    assert v["near_focus"][14] == F(50e-3) / F(0.02) >= 1 and v["near_focus"][13] > 0
    assert v["focus_zero"][14] == np.inf and v["focus_zero"][13] > 0
    assert v["wide"][12] == F(36e-3) / F(32) and v["wide"][13] == F(8e-3) / (F(2) * F(4.0)) and 0 < v["wide"][14] < 1
    assert v["wide_pinhole"][13] == 0 and np.array_equal(np.delete(v["wide_pinhole"], 13), np.delete(v["wide"], 13))
    assert v["tele"][12] == F(24e-3) / F(32) and v["tele"][13] == F(0.8) / (F(2) * F(8.0)) and abs(v["tele"][14] - 0.8 / 160.0) < 1e-6
    assert cc.cases()["portrait"]["res"] == (32, 48) and v["portrait"][12] == F(36e-3) / F(32) != F(36e-3) / F(48)
    assert all(c["res"] == cc.RES for n, c in cc.cases().items() if n != "portrait")
    up, right = v["rolled"][3:6], v["rolled"][6:9]
    assert abs(right[1]) > 0.1 and abs(np.dot(up, right)) < 1e-6 and abs(np.linalg.norm(up) - 1) < 1e-6  # rolled, and still rigid
    assert teapot[7] == 0  # the teapot view's own right has no y
    assert v["look_direction"][14] == F(50e-3) / F(2.0) and np.array_equal(v["look_direction"][0:3], F(cc.EYE))
    assert pinhole[13] == 0 and np.array_equal(np.delete(pinhole, 13), np.delete(teapot, 13))
    for name, (base, k) in cc.SCALED.items():
        b = {"pinhole": pinhole, "wide_pinhole": wide_pinhole}[base]
        # an exact power of two: the f64 product is the f32 value; nothing else changes
        assert np.array_equal(v[name][9:13].astype(np.float64), b[9:13].astype(np.float64) * 2.0 ** k), name
        assert np.array_equal(np.delete(v[name], np.s_[9:13]), np.delete(b, np.s_[9:13])), name
        assert v[name][13] == 0, "a pinhole: the direction is the film point's negative"
    assert (cc.K_MIXED, cc.K_HIGH, cc.K_SUBNORMAL, cc.K_FLUSH) == (-32, 46, -60, -72)
    assert np.array_equal(v["anisotropic"][6:9], teapot[6:9] * F(2)) and abs(np.linalg.norm(v["anisotropic"][6:9]) - 2) < 1e-6
    assert np.array_equal(np.delete(v["anisotropic"], np.s_[6:9]), np.delete(teapot, np.s_[6:9]))
    assert np.array_equal(v["sheared"][3:6], teapot[3:6] + F(0.5) * teapot[6:9]) and abs(np.dot(v["sheared"][3:6], v["sheared"][6:9]) - 0.5) < 1e-6
    assert np.array_equal(np.delete(v["sheared"], np.s_[3:6]), np.delete(teapot, np.s_[3:6]))
    assert v["negative_lens"][13] == -teapot[13] < 0 and np.array_equal(np.delete(v["negative_lens"], 13), np.delete(teapot, 13))


# ---- the windows of rm::ray_dir ---------------------------------------------------------------------------------------------------
def test_scaled_cases_split_the_frame_at_the_windows():
    """ray_math.h takes its short sequences when a whole wave has the sum of squares in [2^-80, 2^80) and every |component| >= 2^-40.
    Counted on the pixel centres from camera_film restated in np.float32: the chosen k put at least 10 % of the frame on either side"""
    wp = cc.base_values("wide_pinhole")
    n = cc.RES[0] * cc.RES[1]
    for k, want in BELOW_COMPONENT.items():
        assert cc.window_counts(cc.scaled(wp, k), cc.RES)[0] == want, k
    for k, want in SUM_ABOVE.items():
        assert cc.window_counts(cc.scaled(wp, k), cc.RES)[1] == want, k
    # k = -32 splits most evenly of -33 ... -30 (906 / 630); k = 46 is the only one with both sides above 10 %
    assert min(BELOW_COMPONENT, key=lambda k: abs(2 * BELOW_COMPONENT[k] - n)) == cc.K_MIXED
    assert [k for k, c in SUM_ABOVE.items() if 10 * c >= n and 10 * (n - c) >= n] == [cc.K_HIGH]
    v = {name: cc.cases()[name]["values"] for name in cc.SCALED}
    assert cc.window_counts(v["scaled_mixed"], cc.RES) == (906, 0, 0)
    assert cc.window_counts(v["scaled_high"], cc.RES) == (0, 1088, 0)
    for name, split in (("scaled_mixed", 906), ("scaled_high", 1088)):
        assert 10 * split >= n and 10 * (n - split) >= n, name
    # for this camera the low edge of the sum is never reached before every pixel has a small component
    assert cc.window_counts(cc.scaled(wp, -34), cc.RES) == (1536, 0, 448)
    # the squares of the two teapot-pinhole cases: all subnormal (non-zero, below 2^-126), all zero
    for name, zero in (("scaled_subnormal", False), ("scaled_flush", True)):
        f = cc.film_at_centres(v[name], cc.RES)
        assert (f != 0).all() and cc.window_counts(v[name], cc.RES) == (n, 0, n)
        with np.errstate(under="ignore"):
            sq = (f * f).astype(F)
        assert (sq == 0).all() if zero else ((sq.max(-1) > 0) & (sq.max(-1) < np.finfo(F).tiny)).all(), name
    # every other finite case lies inside the windows, except sheared's 15 pixels with a small component ... of a lens camera, whose
    # direction adds the lens term: the count is of the film point alone
    for name in cc.FINITE:
        if name not in cc.SCALED and name != "sheared":
            assert cc.window_counts(cc.cases()[name]["values"], cc.cases()[name]["res"]) == (0, 0, 0), name


# ---- the oracle's frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_hits_and_misses(oracle, teapot_oracle_bvh, name):
    """every finite case's 16-spp frame has at least 100 hit and 100 miss pixels; focus_zero and scaled_flush are all alpha 0, no NaN"""
    f = case_frame(oracle, teapot_oracle_bvh, name)
    hit = int((f[..., 3] > 0).sum())
    assert f.shape == cc.cases()[name]["res"][::-1] + (4,) and not np.isnan(f).any()
    assert hit == HITS[name], (name, hit)
    if name in cc.NON_FINITE:
        assert hit == 0 and not f.any()
    else:
        assert hit >= 100 and f[..., 3].size - hit >= 100


def test_non_finite_cases_make_non_finite_rays(oracle):
    """what NON_FINITE means, on the oracle's rays: focus_zero's directions are inf / inf = NaN in every component, scaled_flush's are
    x / 0 = +-inf (the squares are zero, the components are not), with inverses of +-0; the origins are finite"""
    for name, what in (("focus_zero", np.isnan), ("scaled_flush", np.isinf)):
        smp = cc.cases()[name]["sampler"]
        for x, y in ((0, 0), (17, 9), (47, 31)):
            for s in range(4):
                r = oracle.sample_ray(smp, x, y, oracle.lib().mpo_sample_key(C.c_uint64(cc.SEED), cc.RES[0], 16, x, y, s))
                assert what(list(r.d)).all() and np.isfinite(list(r.o)).all(), (name, x, y, s, list(r.d))
                assert np.isnan(list(r.inv)).all() if name == "focus_zero" else (np.array(list(r.inv)) == 0).all()


def test_path_frames_of_every_case_are_free_of_nan(oracle, teapot_oracle_bvh):
    """the path extension's frames too (bit comparisons on the GPU need no NaN rule), and the non-finite cases trace one segment per sample"""
    for name, c in cc.cases().items():
        w, h = c["res"]
        with np.errstate(all="ignore"):
            f, _, _, seg = teapot_oracle_bvh.render_image_paths_mt(c["sampler"], w, h, 16, cc.SEED, cc.DEPTH, cc.TILE, 8)
        assert not np.isnan(f).any(), name
        if name in cc.NON_FINITE:
            assert seg == w * h * 16 and not f[..., 3].any()
        else:
            assert seg > w * h * 16, "paths bounce"


def test_scale_invariance_of_the_oracle(oracle, teapot_oracle_bvh):
    """a power of two is exact while nothing underflows: the frames of wide_pinhole * 2^k, k = -36 ... -30 and 46, are the unscaled
    frame bit for bit"""
    base = case_frame(oracle, teapot_oracle_bvh, "wide_pinhole")
    for name in ("scaled_mixed", "scaled_high"):
        assert np.array_equal(bits(case_frame(oracle, teapot_oracle_bvh, name)), bits(base)), name
    wp = cc.base_values("wide_pinhole")
    for k in range(-36, -29):
        assert np.array_equal(bits(oracle_frame(oracle, teapot_oracle_bvh, cc.scaled(wp, k), cc.RES)), bits(base)), k


def test_subnormal_case_is_a_different_computation(oracle, teapot_oracle_bvh):
    base = oracle_frame(oracle, teapot_oracle_bvh, cc.base_values("pinhole"), cc.RES)
    assert int((base[..., 3] > 0).sum()) == PINHOLE_HITS
    sub = case_frame(oracle, teapot_oracle_bvh, "scaled_subnormal")
    differing = int((bits(sub) != bits(base)).sum())
    print("f32 values differing from the unscaled pinhole frame:", differing)
    assert differing == 1263 > 500


# ---- a wrong kernel would fail ---------------------------------------------------------------------------------------------------
def test_a_kernel_that_dropped_lens_weight_would_fail(oracle, teapot_oracle_bvh):
    """the model of that mistake is the oracle on the same floats with lens_weight = 0"""
    counts = {}
    for name in ("near_focus", "look_direction", "tele"):
        v = cc.cases()[name]["values"].copy()
        assert v[14] != 0 and v[13] != 0
        v[14] = 0
        counts[name] = pixels_differing(oracle_frame(oracle, teapot_oracle_bvh, v, cc.RES), case_frame(oracle, teapot_oracle_bvh, name))
    print("pixels differing without lens_weight:", counts)
    assert all(n > 100 for n in counts.values()), counts


def numpy_build_sampler(cam, res, pixel_scale):
    """camera.rs:123-146 in np.float32 from the camera's basis, with the pixel scale given"""
    center, fwd, up, right = cam.center_forward_up_right()
    rx, ry, ps = F(res[0]), F(res[1]), F(pixel_scale)
    uvx, uvy = ((rx - F(1)) * ps) / F(2), ((ry - F(1)) * ps) / F(2)
    foo = ((-fwd) * F(cam.focal_length) + right * uvx) - up * uvy
    with np.errstate(divide="ignore"):
        tail = [ps, F(cam.focal_length) / (F(2) * F(cam.f_number_)), F(cam.focal_length) / F(cam.focus_distance_)]
    return np.concatenate([center, up, right, foo, tail]).astype(F)


def test_a_kernel_that_sized_the_portrait_sensor_by_its_height_would_fail(oracle, teapot_oracle_bvh):
    c = cc.cases()["portrait"]
    cam, res = c["built"][0], c["res"]
    assert cam.sensor_is_width
    right = numpy_build_sampler(cam, res, F(cam.sensor_size) / F(res[0]))
    assert np.array_equal(bits(right), bits(c["values"])), "the numpy build_sampler is the product's"
    wrong = numpy_build_sampler(cam, res, F(cam.sensor_size) / F(res[1]))
    n = pixels_differing(oracle_frame(oracle, teapot_oracle_bvh, wrong, res), case_frame(oracle, teapot_oracle_bvh, "portrait"))
    print("pixels differing with sensor_size / height:", n)
    assert n > 100


# ---- the unit bounds -------------------------------------------------------------------------------------------------------------
def all_units(res):
    return [(x, x + 1, y, y + 1) for y in range(0, res[1], 2) for x in range(0, res[0], 2)]


def escaping_passes(oracle, case, block, lo, hi, spp=64):
    """test_unit_bounds_cpu.escaping_passes at the case's own width: passes of 16 samples per pixel of the unit with a ray outside [lo, hi]"""
    x0, x1, y0, y1 = block
    L, esc = oracle.lib(), 0
    for p in range(spp // 16):
        rays = []
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                for sub in range(16):
                    r = oracle.sample_ray(case["sampler"], x, y, L.mpo_sample_key(C.c_uint64(cc.SEED), case["res"][0], spp, x, y, p * 16 + sub))
                    rays.append([list(r.o), list(r.inv), list(r.d)])
        v = np.array(rays, F)
        esc += not ((v >= lo) & (v <= hi)).all()
    return esc


@pytest.mark.parametrize("name", cc.NAMES)
def test_unit_bounds_adopt_or_decline(oracle, name):
    """analytic_bounds.corner_header over all 384 units of the frame: the invariants of every adopted header; near_focus and focus_zero
    decline every unit (the corner rays disagree in sign, or are NaN), the open lens at infinite focus, the 8 mm and the 800 mm lens
    adopt at least 300; for wide and inf_focus_open at most 1 % of the passes at 64 spp have a ray outside the adopted bounds"""
    ab = _model()
    c = cc.cases()[name]
    js, margin = ab.jitter_scale(), shipped_margin()
    units = all_units(c["res"])
    assert len(units) == 384
    adopted = passes = esc = 0
    with np.errstate(all="ignore"):
        for blk in units:
            state, lo, hi = ab.corner_header(c["values"], js, *blk, margin)
            if state == 0xFFFFFFFF:
                continue
            adopted += 1
            check_invariants(state, lo, hi)
            if name in ("wide", "inf_focus_open"):
                esc += escaping_passes(oracle, c, blk, lo, hi)
                passes += 4
    assert adopted == ADOPTED[name], (name, adopted)
    if name in ("near_focus", "focus_zero"):
        assert adopted == 0
    if name in ("inf_focus_open", "wide", "tele"):
        assert adopted >= 300
    if passes:
        print(f"{name}: {esc} of {passes} passes escape")
        assert passes == 4 * adopted and esc * 100 <= passes


# ---- the routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(cc.ROUTES))
def test_route_names_are_the_launch_plans(route):
    """the kernels ROUTES expects are what launch_plan.cpp selects for the teapot on six tiles of 16 (both resolutions) under the
    route's options; the cached walk's unit has four passes"""
    row = cc.ROUTES[route]
    o = {**dc.DEFAULTS, **row["opts"]}
    paths = row["api"] in ("paths", "wf")
    out = pp.plan(pp.API[row["api"]], pp.launch(dc.scene_facts("teapot"), 6, cc.TILE, row["spp"], traversal=1 if row.get("traversal") == "groups" else 0,
                                                max_depth=cc.DEPTH if paths else 0, cache=o["packet_mask_cache"], pooled=o["paths_pooled"]))
    assert out.rc == 0, out.error
    if row["api"] == "wf":
        assert row["names"] == {pp.name(out), pp.name(out, "vertex"), pp.name(out, "trace"), "wf_scan_kernel", "wf_scatter_kernel", "wf_accumulate_kernel"}
        assert row["names"] == dc.staged_names("teapot")
    else:
        assert row["names"] == [pp.name(out)]
    if route == "cached":
        in_flight = int(row["names"][0].split("<")[1].split(",")[0])
        assert row["names"][0].endswith(", true>") and row["spp"] // in_flight >= 4
        name, passes = cc.TWO_PASS  # the same frame in two passes: each on the cached kernel of its own sample count
        begin = 0
        for n, kernel in passes:
            assert pp.name(pp.plan(pp.RENDER, pp.launch(dc.scene_facts("teapot"), 6, cc.TILE, row["spp"], passes=(begin, n)))) == kernel
            assert kernel.endswith(", true>")
            begin += n
        assert begin == row["spp"] and name in cc.FINITE
    x0, y0, x1, y1 = cc.RAYS_BLOCK
    assert (x1 - x0, y1 - y0) == (16, 16) and x1 <= min(cc.RES[0], cc.PORTRAIT_RES[0]) and y1 <= min(cc.RES[1], cc.PORTRAIT_RES[1])


# ---- the temporal view ------------------------------------------------------------------------------------------------------------
TEMPORAL_PINHOLES = {"rolled": dict(cc.BUILDERS["rolled"], f_number=INF), "8 mm / 36 mm": cc.BUILDERS["wide_pinhole"],
                     "sensor_width, portrait": dict(cc.BUILDERS["portrait"], f_number=INF)}


@pytest.mark.parametrize("name", list(TEMPORAL_PINHOLES))
def test_temporal_projection_against_the_renderer(oracle, teapot_oracle_bvh, name):
    """test_projection_against_the_renderer for a rolled pinhole, an 8 mm lens on a 36 mm sensor and a sensor_width camera on a
    portrait frame: the mean hit point of every fully covered pixel, projected through temporal_model.view_of of the same camera,
    lands within 0.5 + 1e-3 of its pixel, and TemporalAccumulator.view_of gives the model's 15 floats"""
    spec = TEMPORAL_PINHOLES[name]
    res = spec.get("res", cc.RES)
    cam = cc.product_camera(spec)
    view, smp = tc.oracle_view(oracle, cc.oracle_camera(oracle, spec), res)
    center, forward, up, right = cam.center_forward_up_right()
    want = tm.view_of(center, forward, up, right, cam.focal_length, cam.build_sampler(res).as_array()[12], res).floats()
    got = np.frombuffer(bytes(mp.TemporalAccumulator.view_of(cam, res)), F)
    assert got.size == 15 and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(view.floats()), bits(want))
    pos = aov_pass_model.planes(oracle, teapot_oracle_bvh.intersect, smp, res[0], 8, cc.SEED, (0, 0, res[0], res[1]))["position"]
    full = pos[..., 3] == 1
    assert full.sum() >= 150
    a, u, v = tm.project(view, pos[..., :3])
    yy, xx = np.mgrid[0:res[1], 0:res[0]]
    assert np.all(a[full] > 0)
    du, dv = np.abs(u - xx)[full], np.abs(v - yy)[full]
    print(f"{name}: {int(full.sum())} full pixels, largest |u - x|, |v - y|:", du.max(), dv.max())
    assert du.max() <= 0.5 + 1e-3 and dv.max() <= 0.5 + 1e-3
    assert du.max() > 0.05 and dv.max() > 0.05  # jittered samples: the means are not the pixel centres
