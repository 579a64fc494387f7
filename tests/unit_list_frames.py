"""Frame helpers of tests/test_unit_lists_gpu.py, in a module of their own so that the test depends on no other test module: one
context per tree format, a frame or its feature planes with the kernels that ran, the oracle's images (computed once per case)."""
import functools
import re

import numpy as np

import minipath_amd as mp
from minipath_amd import scenes
from tests import dispatch_cases as dc
from tests import graft_model as gm
from tests.conftest import TEAPOT

SLOTS = (16, 8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_contexts():
    """{slots: context}: the scenes made on each take its tree format at upload"""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    out = {}
    for s in SLOTS:
        c = mp.Context(0)
        c.set_option("packet_tree_slots", s)
        out[s] = c
    return out


def set_options(ctx, **opts):
    for k, v in {**dc.DEFAULTS, **opts}.items():
        ctx.set_option(k, v)


def frame(ctx, obj, cam, st, **opts):
    """one frame through FrameRenderer: (f32 image, u8 image, kernels reported, ray segments)"""
    import torch

    set_options(ctx, **opts)
    try:
        fr = mp.FrameRenderer(mp.Scene(obj), cam, st)
        fr.render()
        names = dc.launched(ctx)
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        return img.cpu().numpy(), img8.cpu().numpy(), names, int(fr.segments.item())
    finally:
        set_options(ctx)


def planes(ctx, obj, cam, st, which):
    """the feature planes `which` of one frame: ({name: image}, kernels reported)"""
    import torch

    set_options(ctx)
    fr = mp.FrameRenderer(mp.Scene(obj), cam, st)
    out = fr.render_aov(**{k: k in which for k in ("shade", "normal", "albedo", "ids")})
    names = dc.launched(ctx)
    img = {k: fr.untile_plane(out[k]).cpu().numpy() for k in which}
    torch.cuda.synchronize()
    return img, names


def check_formats(ctxs, make_obj, cam, st, want, name_re, **opts):
    """the frame under both formats: the scene holds its context's format, the one kernel matches name_re, the image is the
    oracle's bit for bit -- and so the two formats agree"""
    of, ou8 = want
    got = {}
    for slots, ctx in ctxs.items():
        obj = make_obj(ctx)
        assert obj.device_tree(packet=True)[0].shape[1] == slots
        f, u8, names, _ = frame(ctx, obj, cam, st, **opts)
        assert len(names) == 1 and re.fullmatch(name_re, names[0]), (slots, names)
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0, (slots, names, diff)
        assert np.array_equal(u8, ou8), slots
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


@functools.lru_cache(maxsize=None)
def teapot_oracle(oracle, res, spp, seed, ts, depth=0):
    orc = oracle.Bvh.from_obj(TEAPOT)
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    if depth:
        f, u8, _, seg = orc.render_image_paths_mt(smp, *res, spp, seed, depth, ts, 16)
        return f, u8, seg
    f, u8, *_ = orc.render_image_mt(smp, *res, spp, seed, ts, 16)
    return f, u8, None


@functools.lru_cache(maxsize=None)
def evict_oracle_image(oracle, spp):
    smp = oracle.sampler_from_array(scenes.atrium_camera().build_sampler(gm.EVICT_RES).as_array())
    f, u8, *_ = gm.evict_oracle(oracle).render_image_mt(smp, *gm.EVICT_RES, spp, gm.EVICT_SEED, gm.EVICT_TS, 16)
    return f, u8
