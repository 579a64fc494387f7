"""CPU tests of what the seven post-process libraries share: the host scaffold of minipath_amd/post/post_abi.h, compiled into each
library on its own, and the wrappers' helpers minipath_amd/_postlib.py and _traced.py.  Everything here is decided before a library's first HIP
call, so the built libraries are driven without touching a GPU.

A refused call leaves the record of mpX_last_kernels alone: every library's own tests assert it around each refusal they make
(the helpers _call_atrous of test_denoise_cpu, _refused of test_adaptive_cpu, _call_reproject of test_temporal_cpu, _call of
test_secondary_cpu, _downsample and _upsample of test_resample_cpu), so it is not repeated here.  Without a GPU that record is
empty; tests/test_gpu_postlib_common.py asserts the same on a record that holds a kernel, and tools/post_abi_check.hip runs the
record's own rules (distinct names in launch order, left alone by a call that launched nothing) on the host.
"""
import ctypes as C

import pytest
import torch

import minipath_amd as mp
from minipath_amd import adaptive, denoise, lights, resample, secondary, sky, temporal

MP_ERR_INVALID = 1
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
_SAME = (C.c_uint32 * 4)()  # four bytes a call may name twice; every call below is refused before it would touch them


def _refuse_denoise(L):
    return L.mpd_atrous(NO_DEVICE, None, *([None] * 8))


def _refuse_adaptive(L):
    p = C.addressof(_SAME)
    return L.mpa_move_tiles(NO_DEVICE, 1, 1, p, 1, None, p, 1, None, None)


# prefix -> (the wrapper module, a call the library refuses, the reason it gives)
LIBS = {
    "mpd": (denoise, _refuse_denoise, b"settings is NULL"),
    "mpa": (adaptive, _refuse_adaptive, b"d_src == d_dst"),
    "mpt": (temporal, lambda L: L.mpt_check_settings(None), b"settings is NULL"),
    "mps": (secondary, lambda L: L.mps_check_settings(None), b"settings is NULL"),
    "mpr": (resample, lambda L: L.mpr_check_settings(None), b"settings is NULL"),
    "mpl": (lights, lambda L: L.mpl_check_settings(None, None), b"settings is NULL"),
    "mpe": (sky, lambda L: L.mpe_check_settings(None), b"settings is NULL"),
}


# the wrapper module -> (how its missing library's error ends, uses of the wrapper that need the library: each raises as lib() does)
MISSING = {
    denoise: ("the denoiser has no CPU fallback", ()),
    adaptive: ("adaptive sampling has no CPU fallback", ()),
    temporal: ("the reprojection has no CPU fallback", (lambda: mp.TemporalAccumulator((8, 8), "cuda:0"),)),
    secondary: ("the secondary rays have no CPU fallback", ()),
    resample: ("the resampling has no CPU fallback", ()),
    lights: ("the lights have no CPU fallback", ()),
    sky: ("the sky lighting has no CPU fallback", (lambda: mp.gradient_sky(4, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0),)),
}


@pytest.mark.parametrize("mod", MISSING, ids=[m.__name__.rsplit(".", 1)[1] for m in MISSING])
def test_a_missing_library_raises_on_first_use_only(mod, tmp_path):
    """import minipath_amd does not need a post-process library; using one that has not been built is an error, not a fallback"""
    what, uses = MISSING[mod]
    name = mod.LIBRARY.name
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(mod.LIBRARY, "handle", None)
        patch.setattr(mod.LIBRARY, "path", str(tmp_path / f"libminipath_{name}.so"))
        for use in (mod.lib,) + uses:
            with pytest.raises(ImportError) as e:
                use()
            assert str(e.value) == f"{tmp_path}/libminipath_{name}.so is missing: build it with `make -C minipath_amd/csrc` -- {what}"
    assert mod.lib() is mod.LIBRARY.handle and getattr(mod.lib(), f"{mod.LIBRARY.prefix}_last_kernels")  # the real one again


def _fn(prefix, name):
    return getattr(LIBS[prefix][0].lib(), f"{prefix}_{name}")


def _state(prefix):
    """the calling thread's two records of one library, as bytes"""
    need = C.c_size_t()
    assert _fn(prefix, "last_kernels")(None, 0, C.byref(need)) == 0
    buf = C.create_string_buffer(need.value + 1)
    assert _fn(prefix, "last_kernels")(buf, need.value + 1, None) == 0
    return _fn(prefix, "last_error")(), buf.value


@pytest.mark.parametrize("prefix", LIBS)
def test_a_failing_call_touches_its_own_library_alone(prefix):
    """each shared object has records of its own: a refusal in one changes no other library's last error or last kernels"""
    for p, (mod, refuse, why) in LIBS.items():
        assert refuse(mod.lib()) == MP_ERR_INVALID and _fn(p, "last_error")() == why
    before = {p: _state(p) for p in LIBS}
    assert _fn(prefix, "last_kernels")(None, 4, None) == MP_ERR_INVALID  # another reason than any library holds
    assert _fn(prefix, "last_error")() == b"NULL argument"
    for p in LIBS:
        if p != prefix:
            assert _state(p) == before[p], p
    assert _state(prefix)[1] == before[prefix][1]  # the refused call left its own kernel record alone


@pytest.mark.parametrize("prefix", LIBS)
def test_last_kernels_buffer_protocol(prefix):
    fn = _fn(prefix, "last_kernels")
    need = C.c_size_t(99)
    assert fn(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(LIBS[prefix][0].last_kernels()))  # cap 0: the size alone
    assert fn(None, 4, None) == MP_ERR_INVALID and _fn(prefix, "last_error")() == b"NULL argument"
    buf = C.create_string_buffer(b"\xff" * 8, 8)
    assert fn(buf, 1, None) == 0 and buf.raw == b"\x00" + b"\xff" * 7  # cap 1: the terminating 0 alone


# ---- the wrappers' plane checks: the texts are those of the wrappers before they shared expect_plane ----------------------------
def _wrapper(cls, **attrs):
    """a wrapper object for 5 x 3 planes on cuda:0 without its library or a GPU: _plane reads these attributes alone"""
    o = object.__new__(cls)
    o.device, o.device_id, o.width, o.height = torch.device("cuda", 0), 0, 5, 3
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


PLANE_CASES = [
    (denoise.AtrousDenoiser, {}, "color", {}, "color: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"),
    (temporal.TemporalAccumulator, {}, "color", {}, "color: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"),
    (temporal.TemporalAccumulator, {}, "ids", dict(dtypes=(torch.int32, torch.uint32)),
     "ids: a contiguous int32 or uint32 [3, 5, 4] tensor on cuda:0 is expected"),
    (secondary.SecondaryVisibility, {}, "position", {}, "position: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"),
    (lights.LocalLights, {}, "position", {}, "position: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"),
    (sky.SkyLight, {}, "position", {}, "position: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"),
    (resample.GuidedResampler, dict(low_resolution=(3, 2)), "position", {},
     "position: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"),
    (resample.GuidedResampler, dict(low_resolution=(3, 2)), "extra[0]", dict(words=True),
     "extra[0]: a contiguous float32 or int32 [3, 5, 4] tensor on cuda:0 is expected"),
    (resample.GuidedResampler, dict(low_resolution=(3, 2)), "color_lo", dict(low=True),
     "color_lo: a contiguous float32 [2, 3, 4] tensor on cuda:0 is expected"),
]


@pytest.mark.parametrize("cls,attrs,name,kw,text", PLANE_CASES, ids=[f"{c[0].__name__}-{c[2]}" for c in PLANE_CASES])
def test_plane_refusals_read_as_before(cls, attrs, name, kw, text):
    """one tensor of a wrong dtype and one of a wrong shape per wrapper and message form (adaptive.py checks no planes)"""
    o = _wrapper(cls, **attrs)
    for t in (torch.zeros((3, 5, 4), dtype=torch.float64), torch.zeros((5, 3, 4), dtype=torch.float32)):
        with pytest.raises(ValueError) as e:
            o._plane(t, name, **kw)
        assert str(e.value) == text


def test_none_passes_where_a_plane_is_optional():
    """denoise and temporal hand None through (their nullable planes); secondary, lights, sky and resample refuse it like any
    non-tensor"""
    assert _wrapper(denoise.AtrousDenoiser)._plane(None, "albedo") is None
    assert _wrapper(temporal.TemporalAccumulator)._plane(None, "variance") is None
    for cls, attrs in ((secondary.SecondaryVisibility, {}), (lights.LocalLights, {}), (sky.SkyLight, {}),
                       (resample.GuidedResampler, dict(low_resolution=(3, 2)))):
        with pytest.raises(ValueError) as e:
            _wrapper(cls, **attrs)._plane(None, "position")
        assert str(e.value) == "position: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"
