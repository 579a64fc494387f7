"""CPU tests of the a-trous denoiser: properties of the numpy model (tests/denoise_model.py, the restatement of
include/minipath_denoise.h that the GPU tests compare bits against), and what libminipath_denoise.so decides before its first HIP
call -- every refusal, the scratch size, the struct size -- through the built library without touching a GPU."""
import ctypes as C
import inspect
import itertools

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import denoise as dn
from tests import denoise_model as m
from tests.conftest import TEAPOT
from tests.denoise_model import F, bits

MP_ERR_INVALID = 1
SENTINEL = 0x5A5A5A5A


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 7])
@pytest.mark.parametrize("with_variance", [False, True])
def test_orthogonal_halves_do_not_mix(k, with_variance):
    """two halves with orthogonal normals: every weight across the edge is exactly 0, so each half is filtered as if alone"""
    w, h = 22, 13
    p = m.synthetic(w, h, 5)
    p["normal"][:, : w // 2, :3] = (1, 0, 0)
    p["normal"][:, w // 2:, :3] = (0, 1, 0)
    kw = dict(iterations=4, k=k, sigma_depth=0.5, sigma_luminance=0.7)
    var = p["variance"] if with_variance else None
    whole = m.atrous(p["color"], p["normal"], variance=var, **kw)
    for sl in (slice(0, w // 2), slice(w // 2, w)):
        alone = m.atrous(p["color"][:, sl], p["normal"][:, sl], variance=None if var is None else var[:, sl], **kw)
        if with_variance:
            assert _same(whole[0][:, sl], alone[0]) and _same(whole[1][:, sl], alone[1])
        else:
            assert _same(whole[:, sl], alone)


def test_misses_pass_through_and_are_never_taps():
    p = m.synthetic(31, 17, 9)
    miss = p["color"][..., 3] == 0
    assert 0 < miss.sum() < miss.size
    kw = dict(albedo=p["albedo"], variance=p["variance"], iterations=5, k=2, sigma_depth=0.5, sigma_luminance=2.0, demodulate=True)
    out, vout = m.atrous(p["color"], p["normal"], **kw)
    assert _same(out[miss], p["color"][miss]) and _same(vout[miss][:, 0], p["variance"][miss][:, 0])
    assert np.all(np.isfinite(out[~miss])) and np.all(np.abs(out[~miss]) < 1e3)  # the 1e30 colours of the misses did not leak
    other = {k: v.copy() for k, v in p.items()}
    other["color"][miss, :3] = np.nan  # what a miss holds does not matter to anybody else
    other["normal"][miss] = 0
    other["variance"][miss, 0] = np.inf
    kw.update(albedo=other["albedo"], variance=other["variance"])
    out2, vout2 = m.atrous(other["color"], other["normal"], **kw)
    assert _same(out[~miss], out2[~miss]) and _same(vout[~miss], vout2[~miss])
    assert np.all(vout[..., 1:] == 0)


def test_one_pass_is_the_b3_spline():
    """k = 0, equal normals, huge sigmas: every weight is hw, so one pass is the 5 x 5 B3 spline renormalised at the borders"""
    w, h = 19, 11
    rng = np.random.default_rng(3)
    color = rng.random((h, w, 4)).astype(F)
    color[..., 3] = 1
    nd = np.zeros((h, w, 4), F)
    nd[..., 2] = 1
    nd[..., 3] = rng.random((h, w)).astype(F) * 10
    out = m.atrous(color, nd, iterations=1, k=0, sigma_depth=1e30, sigma_luminance=1e30)
    h5 = np.array([1, 4, 6, 4, 1], np.float64) / 16
    want = np.zeros((h, w, 3))
    for y, x in itertools.product(range(h), range(w)):
        acc, tot = np.zeros(3), 0.0
        for dy, dx in itertools.product(range(-2, 3), repeat=2):
            if 0 <= y + dy < h and 0 <= x + dx < w:
                acc += h5[dy + 2] * h5[dx + 2] * color[y + dy, x + dx, :3].astype(np.float64)
                tot += h5[dy + 2] * h5[dx + 2]
        want[y, x] = acc / tot
    assert np.max(np.abs(out[..., :3] - want)) <= 1e-6
    assert _same(out[..., 3], color[..., 3])


def test_variance_from_moments_against_f64():
    rng = np.random.default_rng(4)
    h, w, n = 12, 15, 16
    alpha = rng.integers(0, n + 1, (h, w)) / n
    mean = rng.random((h, w))
    spread = rng.random((h, w)) * 0.1
    spread[rng.random((h, w)) < 0.2] = 0  # q == m*m up to rounding: the clamp at 0
    shade = np.zeros((h, w, 4), F)
    sq = np.zeros((h, w, 4), F)
    shade[..., 0], shade[..., 3] = mean * alpha, alpha
    sq[..., 0], sq[..., 3] = (mean * mean + spread) * alpha, alpha
    got = m.variance_from_moments(shade, sq, n)
    assert np.all(got[..., 1:] == 0) and np.all(got[alpha == 0] == 0) and np.all(got[..., 0] >= 0)
    a64, s64, q64 = shade[..., 3].astype(np.float64), shade[..., 0].astype(np.float64), sq[..., 0].astype(np.float64)
    hit = a64 != 0
    m64, qq = s64[hit] / a64[hit], q64[hit] / a64[hit]
    want = np.maximum(qq - m64 * m64, 0) / (n * a64[hit])
    # m and q carry one rounding each, m*m two more, the difference one (absolute, on numbers of size q + m*m), the two products and
    # the quotient of the end three relative ones: 6 units of 2^-24 on (q + m*m) / (n * alpha) covers all of it
    bound = 6 * 2.0 ** -24 * (qq + m64 * m64) / (n * a64[hit])
    assert np.all(np.abs(got[..., 0][hit] - want) <= bound)


def test_default_sigmas_help_on_the_teapot():
    """the usefulness condition of the GPU suite, on the CPU: the oracle's 8-spp path-traced teapot (max_depth 3, 96 x 64) filtered by
    the model with the guides of the same primary rays and the defaults AtrousDenoiser ships is closer to the 512-spp frame"""
    from oracle import pyoracle as po
    from tests import aov_pass_model

    w, h, seed = 96, 64, 0x5EED
    b = po.Bvh.from_obj(TEAPOT)
    s = po.build_sampler(po.teapot_camera(), w, h)
    noisy = b.render_image_paths_mt(s, w, h, 8, seed, 3, tile=32)[0]
    ref = b.render_image_paths_mt(s, w, h, 512, seed, 3, tile=32)[0]
    guides = aov_pass_model.planes(po, lambda r: b.intersect(r), s, w, 8, seed, (0, 0, w, h))
    d = {k: v.default for k, v in inspect.signature(mp.AtrousDenoiser.__init__).parameters.items()}
    out = m.atrous(noisy, guides["normal"], albedo=guides["albedo"], iterations=d["iterations"], k=d["sigma_normal_pow2"],
                   sigma_depth=d["sigma_depth"], sigma_luminance=d["sigma_luminance"], demodulate=True)

    def mse(a):
        return float(np.mean((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2))
    print("mse 8 spp", mse(noisy), "denoised", mse(out))
    assert mse(out) < mse(noisy)


# ---- the library, before its first HIP call ------------------------------------------------------------------------------------
W, H = 6, 5


def _settings(**kw):
    v = dict(struct_size=C.sizeof(dn.DenoiseSettings), width=W, height=H, iterations=3, sigma_normal_pow2=7.0, sigma_depth=0.5,
             sigma_luminance=1.0, flags=0)
    v.update(kw)
    return dn.DenoiseSettings(**v)


def test_struct_size_and_symbols():
    L = dn.lib()
    assert L.mpd_settings_size() == C.sizeof(dn.DenoiseSettings) == 32
    assert mp.AtrousDenoiser is dn.AtrousDenoiser


def test_scratch_floats():
    L = dn.lib()
    assert L.mpd_scratch_floats(C.byref(_settings()), 0) == 2 * H * W * 4
    assert L.mpd_scratch_floats(C.byref(_settings()), 1) == 4 * H * W * 4
    assert L.mpd_scratch_floats(C.byref(_settings(width=1920, height=1080, iterations=1)), 1) == 4 * 1080 * 1920 * 4
    assert L.mpd_scratch_floats(C.byref(_settings(width=1 << 20, height=1 << 20)), 1) == 16 << 40
    assert L.mpd_scratch_floats(None, 0) == 0
    assert L.mpd_scratch_floats(C.byref(_settings(iterations=0)), 0) == 0
    assert L.mpd_scratch_floats(C.byref(_settings(width=0)), 1) == 0


NAN = float("nan")
BAD_SETTINGS = [dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=(1 << 20) + 1), dict(iterations=0), dict(iterations=9),
                dict(sigma_depth=0.0), dict(sigma_depth=-1.0), dict(sigma_depth=NAN), dict(sigma_luminance=0.0),
                dict(sigma_luminance=-0.5), dict(sigma_luminance=NAN), dict(sigma_normal_pow2=-1.0), dict(sigma_normal_pow2=9.0),
                dict(sigma_normal_pow2=2.5), dict(sigma_normal_pow2=NAN), dict(struct_size=0), dict(struct_size=28), dict(flags=2),
                dict(flags=1)]  # the last: DEMODULATE, and the call below passes no albedo
ARGS = ("color", "normal", "albedo", "variance", "scratch", "out", "variance_out")
BAD_ARGS = [dict(color=None), dict(normal=None), dict(scratch=None), dict(out=None), dict(variance=None), dict(device=-1),
            dict(out="color"), dict(out="scratch"), dict(variance_out="out"), dict(variance_out="variance"), dict(settings=None)]


def _buffers():
    return {k: np.full(4 * H * W * 4, SENTINEL, np.uint32) for k in ARGS}


NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched


def _call_atrous(st, bufs, device=NO_DEVICE, **replace):
    ptr = {k: bufs[k].ctypes.data for k in ARGS}
    for k, v in replace.items():
        ptr[k] = None if v is None else ptr[v]
    before = dn.last_kernels()
    rc = dn.lib().mpd_atrous(device, None if st is None else C.byref(st), *[ptr[k] for k in ARGS], None)
    assert dn.last_kernels() == before  # nothing was launched
    for k in ARGS:
        assert np.all(bufs[k] == SENTINEL), k  # nothing was written (host memory here: a launch would not even get this far)
    return rc


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_atrous_refuses_settings(bad):
    replace = dict(albedo=None) if bad.get("flags") == 1 else {}
    assert _call_atrous(_settings(**bad), _buffers(), **replace) == MP_ERR_INVALID
    assert dn.lib().mpd_last_error()


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_atrous_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _call_atrous(st, _buffers(), **bad) == MP_ERR_INVALID
    assert dn.lib().mpd_last_error()


@pytest.mark.parametrize("bad", [dict(shade=None), dict(shade_sq=None), dict(var=None), dict(width=0), dict(height=0), dict(count=0),
                                 dict(device=-1), dict(var="shade"), dict(width=(1 << 20) + 1)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_moments_refuses(bad):
    bufs = {k: np.full(H * W * 4, SENTINEL, np.uint32) for k in ("shade", "shade_sq", "var")}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    for k in ("shade", "shade_sq", "var"):
        if k in bad:
            ptr[k] = None if bad[k] is None else ptr[bad[k]]
    before = dn.last_kernels()
    rc = dn.lib().mpd_variance_from_moments(bad.get("device", NO_DEVICE), bad.get("width", W), bad.get("height", H), bad.get("count", 8),
                                            ptr["shade"], ptr["shade_sq"], ptr["var"], None)
    assert rc == MP_ERR_INVALID and dn.lib().mpd_last_error()
    assert dn.last_kernels() == before and all(np.all(v == SENTINEL) for v in bufs.values())


def test_last_kernels_buffer_protocol():
    L = dn.lib()
    need = C.c_size_t(99)
    assert L.mpd_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(dn.last_kernels()))
    assert L.mpd_last_kernels(None, 4, None) == MP_ERR_INVALID
