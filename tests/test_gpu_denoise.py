"""GPU tests of the a-trous denoiser (include/minipath_denoise.h, minipath_amd.AtrousDenoiser).  Every comparison is on f32 bit
patterns against the numpy model (tests/denoise_model.py) with zero differences allowed, and every case pins the kernels the call
reported: synthetic planes at the sizes where the lattice tiling can go wrong, sentinels around every buffer, the renderer's own
planes, two streams, and the condition that makes the filter worth having (a denoised 8-spp frame is closer to the 512-spp one)."""
import numpy as np
import pytest

import minipath_amd as mp
from tests import denoise_model as m
from tests.conftest import TEAPOT
from tests.denoise_model import F, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
K_PLAIN, K_VAR, K_MOMENTS = "atrous_kernel<false>", "atrous_kernel<true>", "moments_kernel"
# (width, height, iterations): one pixel; every non-centre tap outside from step 4 on; no multiple of the 16-pixel tile; step 16 with
# several lattice classes per block row and halos across the right and bottom edges; either side of the tile edge; all 8 passes
SHAPES = [(1, 1, 3), (7, 5, 5), (37, 23, 3), (70, 33, 5), (16, 16, 2), (17, 17, 2), (9, 6, 8)]
SIGMAS = dict(sigma_depth=0.4, sigma_luminance=0.8)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


_planes = {}


def planes(w, h):
    """the synthetic planes of a shape, made once and never changed"""
    if (w, h) not in _planes:
        _planes[w, h] = m.synthetic(w, h, 1000 * w + h)
    return _planes[w, h]


def _same(got, want, what):
    diff = int(np.sum(bits(got) != bits(want)))
    assert diff == 0, (what, diff)


def _run(torch, p, w, h, iterations, k, variance, demodulate, **kw):
    dev = {n: torch.from_numpy(a).cuda() for n, a in p.items()}
    dn = mp.AtrousDenoiser((w, h), 0, iterations=iterations, sigma_normal_pow2=k, demodulate_albedo=demodulate, **SIGMAS, **kw)
    got = dn.denoise(dev["color"], dev["normal"], albedo=dev["albedo"] if demodulate else None, variance=dev["variance"] if variance else None)
    names = dn.last_kernels()
    torch.cuda.synchronize()
    for n, a in p.items():  # the inputs are only read
        _same(dev[n].cpu().numpy(), a, ("input changed", n))
    return got, names


@pytest.mark.parametrize("k", [0, 7])
@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("variance", [False, True], ids=["novar", "var"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_it%d" % s)
def test_synthetic_planes_match_the_model(torch, shape, variance, demodulate, k):
    w, h, iterations = shape
    p = planes(w, h)
    got, names = _run(torch, p, w, h, iterations, k, variance, demodulate)
    want = m.atrous(p["color"], p["normal"], albedo=p["albedo"], variance=p["variance"] if variance else None, iterations=iterations, k=k,
                    demodulate=demodulate, **SIGMAS)
    if variance:
        assert names == [K_VAR]
        _same(got[0].cpu().numpy(), want[0], "colour")
        _same(got[1].cpu().numpy(), want[1], "variance")
    else:
        assert names == [K_PLAIN]
        _same(got.cpu().numpy(), want, "colour")


def test_variance_from_moments_matches_the_model(torch):
    w, h, n = 37, 23, 12
    rng = np.random.default_rng(7)
    alpha = (rng.integers(0, n + 1, (h, w)) / n).astype(F)
    shade, sq = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    c = rng.random((h, w, n)).astype(F) * (rng.random((h, w, n)) < alpha[..., None])
    shade[..., 0], sq[..., 0] = c.mean(-1), (c * c).mean(-1)
    shade[..., 3] = sq[..., 3] = alpha
    shade[alpha == 0, 0] = 5  # not read into the result: alpha == 0 gives 0
    dn = mp.AtrousDenoiser((w, h), 0)
    got = dn.variance_from_moments(torch.from_numpy(shade).cuda(), torch.from_numpy(sq).cuda(), n)
    assert dn.last_kernels() == [K_MOMENTS]
    _same(got.cpu().numpy(), m.variance_from_moments(shade, sq, n), "variance")


def _guarded(torch, a, pad=4096):
    """a copy of the host array (or `a` floats of nothing) in the middle of a larger tensor of sentinels: (whole, view)"""
    n = a if isinstance(a, int) else a.size
    whole = torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    view = whole[pad:pad + n]
    if not isinstance(a, int):
        view.copy_(torch.from_numpy(a.reshape(-1)))
        view = view.view(a.shape)
    return whole, view


@pytest.mark.parametrize("shape", [(37, 23, 3), (70, 33, 5)], ids=lambda s: "%dx%d_it%d" % s)
def test_nothing_is_written_outside_the_buffers(torch, shape):
    w, h, iterations = shape
    p = planes(w, h)
    pad = 4096
    inputs = {n: _guarded(torch, a, pad) for n, a in p.items()}
    want = m.atrous(p["color"], p["normal"], albedo=p["albedo"], variance=p["variance"], iterations=iterations, k=2, demodulate=True, **SIGMAS)
    dn0 = mp.AtrousDenoiser((w, h), 0, iterations=iterations, sigma_normal_pow2=2, demodulate_albedo=True, **SIGMAS)
    scratch = _guarded(torch, dn0.scratch_floats(True), pad)
    out, vout = _guarded(torch, h * w * 4, pad), _guarded(torch, h * w * 4, pad)
    dn = mp.AtrousDenoiser((w, h), 0, iterations=iterations, sigma_normal_pow2=2, demodulate_albedo=True, scratch=scratch[1], **SIGMAS)
    view = {n: v[1] for n, v in inputs.items()}
    got = dn.denoise(view["color"], view["normal"], albedo=view["albedo"], variance=view["variance"], out=out[1].view(h, w, 4),
                     variance_out=vout[1].view(h, w, 4))
    assert dn.last_kernels() == [K_VAR]
    # the same without a variance plane, into the same guarded buffers: half the scratch
    got2 = dn.denoise(view["color"], view["normal"], albedo=view["albedo"]).cpu().numpy()
    assert dn.last_kernels() == [K_PLAIN]
    torch.cuda.synchronize()
    _same(got[0].cpu().numpy(), want[0], "colour")
    _same(got[1].cpu().numpy(), want[1], "variance")
    _same(got2, m.atrous(p["color"], p["normal"], albedo=p["albedo"], iterations=iterations, k=2, demodulate=True, **SIGMAS), "colour, no variance")
    for name, (whole, _) in list(inputs.items()) + [("scratch", scratch), ("out", out), ("variance_out", vout)]:
        raw = whole.view(torch.int32).cpu().numpy()
        assert np.all(raw[:pad] == SENTINEL) and np.all(raw[-pad:] == SENTINEL), name
    for n, a in p.items():
        _same(view[n].cpu().numpy(), a, ("input changed", n))


def _teapot(ctx):
    return mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx)), mp.Camera.teapot_view()


def test_the_renderers_own_planes(torch):
    """teapot, 72 x 40 in tiles of 32, 16 spp: render_aov_pass -> untile_plane -> variance_from_moments -> denoise, against the model
    on the same planes copied to the host"""
    ctx = mp.Context(0)
    scene, cam = _teapot(ctx)
    st = mp.RenderSettings(32, 16, (72, 40), seed=3)
    fr = mp.FrameRenderer(scene, cam, st)
    pl = fr.new_aov_planes(ids=False, shade_sq=True)
    fr.render_aov_pass(pl)
    img = {n: fr.untile_plane(t) for n, t in pl.items()}
    dn = mp.AtrousDenoiser(st.resolution, fr.device, demodulate_albedo=True)
    var = dn.variance_from_moments(img["shade"], img["shade_sq"], st.sample_count)
    assert dn.last_kernels() == [K_MOMENTS]
    out, vout = dn.denoise(img["shade"], img["normal"], albedo=img["albedo"], variance=var)
    assert dn.last_kernels() == [K_VAR]
    host = {n: t.cpu().numpy() for n, t in img.items()}
    assert 0 < np.count_nonzero(host["shade"][..., 3]) < 72 * 40  # hits and misses
    hvar = m.variance_from_moments(host["shade"], host["shade_sq"], st.sample_count)
    _same(var.cpu().numpy(), hvar, "variance from moments")
    assert hvar[..., 0].max() > 0
    d = dn.settings
    want = m.atrous(host["shade"], host["normal"], albedo=host["albedo"], variance=hvar, iterations=d.iterations, k=int(d.sigma_normal_pow2),
                    sigma_depth=d.sigma_depth, sigma_luminance=d.sigma_luminance, demodulate=True)
    _same(out.cpu().numpy(), want[0], "colour")
    _same(vout.cpu().numpy(), want[1], "variance")
    assert np.sum(bits(want[0]) != bits(host["shade"])) > 72 * 40 // 8  # the filter did something


def test_a_denoised_8spp_frame_is_closer_to_512spp(torch):
    """teapot with the path extension (max_depth 3), 96 x 64: the 8-spp frame filtered with its own guides, albedo demodulated and
    the default sigmas, has a strictly lower mean squared error against the 512-spp frame of the same seed than it had before"""
    ctx = mp.Context(0)
    scene, cam = _teapot(ctx)
    frames = {}
    for spp in (8, 512):
        fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(32, spp, (96, 64), seed=0x5EED, max_depth=3))
        frames[spp] = fr.untile(fr.render(), want_u8=False)[0]
        if spp == 8:
            pl = fr.new_aov_planes(shade=False, ids=False)
            fr.render_aov_pass(pl)
            normal, albedo = fr.untile_plane(pl["normal"]), fr.untile_plane(pl["albedo"])
    dn = mp.AtrousDenoiser((96, 64), 0, demodulate_albedo=True)
    out = dn.denoise(frames[8], normal, albedo=albedo)
    assert dn.last_kernels() == [K_PLAIN]
    ref = frames[512].cpu().numpy()[..., :3].astype(np.float64)

    def mse(t):
        return float(np.mean((t.cpu().numpy()[..., :3].astype(np.float64) - ref) ** 2))
    before, after = mse(frames[8]), mse(out)
    print("mse against 512 spp: 8 spp", before, "denoised", after)
    assert after < before


def test_two_streams(torch):
    """two denoisers on two torch streams: each result is its own model's"""
    cases = [(37, 23, 3, 7, True), (70, 33, 5, 0, False)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = [{n: torch.from_numpy(a).cuda() for n, a in planes(w, h).items()} for w, h, _, _, _ in cases]
    dns = [mp.AtrousDenoiser((w, h), 0, iterations=it, sigma_normal_pow2=k, **SIGMAS) for w, h, it, k, _ in cases]
    torch.cuda.synchronize()
    got = [None, None]
    for rounds in range(3):  # interleaved, so the two have work in flight together
        for i, (s, d, dn, c) in enumerate(zip(streams, dev, dns, cases)):
            with torch.cuda.stream(s):
                got[i] = dn.denoise(d["color"], d["normal"], variance=d["variance"] if c[4] else None)
                assert dn.last_kernels() == [K_VAR if c[4] else K_PLAIN]
    torch.cuda.synchronize()
    for i, (w, h, it, k, var) in enumerate(cases):
        p = planes(w, h)
        want = m.atrous(p["color"], p["normal"], variance=p["variance"] if var else None, iterations=it, k=k, **SIGMAS)
        if var:
            _same(got[i][0].cpu().numpy(), want[0], "colour, stream 0")
            _same(got[i][1].cpu().numpy(), want[1], "variance, stream 0")
        else:
            _same(got[i].cpu().numpy(), want, "colour, stream 1")
