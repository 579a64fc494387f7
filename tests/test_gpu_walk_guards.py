"""GPU parity tests (-m gpu) of the cached packet walk's wave-level guards, bit-exact against the oracle with the per-unit mask cache
forced on and off: the short reciprocal of the triangle determinant (taken only when every lane's |det| lies in [2^-94, 2^125], the
whole wave divides otherwise), the branch-free pass-entry check (mask_cache_ray_ok and the containment test of the unit's bounds),
and the acceptance test written with minNum (hits at u = v = t = +-0)."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp

pytestmark = pytest.mark.gpu
RES = (96, 64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render_both(oracle, pos, nrm, tex, tri, eye, at, fnum, spp, seed, sflight=0):
    """The oracle's image of the view, then the GPU's (mp.render, through the C ABI) with the mask cache on and off; returns the
    oracle image."""
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    oc = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(oc))
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*eye), oracle.vec3(*at), oracle.vec3(0, 1, 0))
    oc.f_number = fnum
    of, ou8, _, _, _ = orc.render_image_mt(oracle.build_sampler(oc, *RES), RES[0], RES[1], spp, seed, 32, 8)
    for mode in (1, 0):
        c = mp.Context(0)
        c.set_option("packet_mask_cache", mode)
        if sflight:
            c.set_option("packet_samples_in_flight", sflight)
        scene = mp.Scene(mp.TriangleBvh.build(pos, nrm, tex, tri, c))
        cam = mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(fnum)
        job = mp.render(scene, cam, mp.RenderSettings(32, spp, RES, seed=seed))
        job.wait()
        got = job.image_f32()
        assert np.array_equal(bits(got), bits(of)), (eye, fnum, mode, int(np.sum(bits(got) != bits(of))))
        assert np.array_equal(job.image(), ou8), (eye, fnum, mode)
    return of


def scaled(scale, pos, *pts):
    p = (pos * np.float32(scale)).astype(np.float32)
    return (p,) + tuple(tuple(float(np.float32(x) * np.float32(scale)) for x in q) for q in pts)


@pytest.mark.parametrize("scale", [2.0 ** -46, 2.0 ** -44, 1.0, 2.0 ** 25])
def test_determinant_window(oracle, scale):
    """Scenes whose triangle determinants fall around and below the short reciprocal's window (the stand-in scaled by 2^-46: |det|
    mostly below 2^-94, most waves divide; by 2^-44: waves of both kinds), inside it, and far above 2^40 with coordinates near the
    2^30 cap of the triangle masks.  Pinhole views (the lens radius does not scale with the scene, so it is made negligible)."""
    from minipath_amd import scenes

    pos, nrm, tex, tri = scenes.atrium(1, 0.08)
    p, eye, at = scaled(scale, pos, (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0))
    of = render_both(oracle, p, nrm, tex, tri, eye, at, 1e30, 64, 17)
    assert np.count_nonzero(of[..., 3]) > 200  # the view does hit the scene


def test_passes_leaving_the_bounds(oracle):
    """Units of 16 passes through a wide lens and through a pinhole, 16 samples in flight: passes whose rays leave the unit's bounds
    (in origin or in direction, by few lanes) widen them, clear the cache and go on, and passes inside take the cache."""
    from minipath_amd import scenes

    pos, nrm, tex, tri = scenes.atrium(1, 0.08)
    for fnum in (1.2, 1e30):
        of = render_both(oracle, pos, nrm, tex, tri, (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0), fnum, 256, 29, sflight=16)
        assert np.count_nonzero(of[..., 3]) > 200


def test_hits_at_signed_zero(oracle):
    """The eye placed exactly on a vertex of the mesh: for the triangles that share it, s = o - v0 = 0, so u and v are +-0 (the sign
    follows det's and the numerators' zero signs) and t = +-0, and such a triangle is accepted at t = 0 exactly when the reference's
    `>= 0` tests accept it.  Every pixel's first hit is decided there."""
    from minipath_amd import scenes

    pos, nrm, tex, tri = scenes.atrium(1, 0.08)
    p = pos.reshape(-1, 3)
    # a vertex all of whose coordinates are of magnitude >= 1: the pinhole's lens offset rounds away, so every ray starts on it
    ok = np.nonzero(np.all(np.abs(p) >= 1.0, axis=1))[0]
    assert ok.size > 0
    v = p[ok[len(ok) // 2]]
    eye = tuple(float(x) for x in v)
    at = (float(v[0]) + 3.0, float(v[1]) + 0.25, float(v[2]) - 1.0)
    of = render_both(oracle, pos, nrm, tex, tri, eye, at, 1e30, 32, 5)
    assert np.count_nonzero(of[..., 3]) > 200
