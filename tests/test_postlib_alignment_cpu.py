"""CPU tests of the alignment the six post-process libraries ask of their buffers (minipath_amd/post/post_abi.h: all_aligned):
a plane is read and written as 16-byte pixels, a ray array or a pick array as 32-bit words, and a pointer that is not so aligned
is refused with MP_ERR_INVALID before the library's first HIP call -- what the hardware would do with it is not this project's to
define.  Every entry point that takes a buffer is called with nothing wrong but one pointer, 4, 8 or 12 bytes past a 16-byte
boundary for a plane and 1, 2 or 3 bytes past a word for a ray array; the same call with every pointer aligned gets as far as the
device (which does not exist).  The buffers are host memory with a sentinel in every word: a call accepted by mistake would be
refused by the runtime (NO_DEVICE), and nothing may be written either way.  The wrappers' own check (_postlib.expect_plane) is
tested on a stand-in tensor that claims to live on a GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from minipath_amd import _postlib
from minipath_amd import adaptive as ad
from minipath_amd import denoise as dn
from minipath_amd import lights as ll
from minipath_amd import resample as rs
from minipath_amd import secondary as sv
from minipath_amd import temporal as tp

MP_ERR_INVALID, MP_ERR_HIP = 1, 4
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
SENTINEL = 0xA5A5A5A5
W, H, B, NL, F = 6, 5, 3, 2, 2  # image, samples per batch, lights, resampling factor
TS, SLOTS = 4, 3                # adaptive: tile size and slots
# Every buffer of a call gets a region of its own in one arena, its first byte on a 16-byte boundary; a region is larger than the
# largest buffer any call states (the denoiser's scratch: four planes) by more than the 12 bytes a pointer is moved, so a moved
# buffer overlaps nothing and the refusal can only be the alignment's.
REGION = 4 * H * W * 16 + 64


def _lights_settings():
    st = ll.LightsSettings(struct_size=C.sizeof(ll.LightsSettings), width=W, height=H, flags=0, sample_count=8, sample_begin=2, batch=B,
                           light_count=NL, seed=1, bias=1e-4, margin=0.0)
    st.eye[:] = (0.0, 0.0, 5.0)
    return st


_TABLE = ll.light_table([((0.0, 1.0, 2.0), 0.0, (1.0, 1.0, 1.0)), ((3.0, -1.0, 0.5), 0.25, (0.0, 2.0, 0.0))])


def _secondary_settings():
    st = sv.SecondarySettings(struct_size=C.sizeof(sv.SecondarySettings), width=W, height=H, mode=0, flags=0, sample_count=8, sample_begin=2,
                              batch=B, seed=1, radius=1.0, bias=1e-4, spread=0.0)
    st.eye[:], st.light[:] = (0.0, 0.0, 5.0), (0.0, 0.6, 0.8)
    return st


def _denoise_settings():
    return dn.DenoiseSettings(struct_size=C.sizeof(dn.DenoiseSettings), width=W, height=H, iterations=3, sigma_normal_pow2=7.0,
                              sigma_depth=0.5, sigma_luminance=1.0, flags=1)  # DEMODULATE: albedo is read too


def _temporal_settings():
    return tp.TemporalSettings(struct_size=C.sizeof(tp.TemporalSettings), width=W, height=H, flags=0, sigma_position=0.01, normal_min=0.9,
                               max_history=32.0, alpha_color=0.2, alpha_moments=0.2, min_variance_history=4.0)


def _resample_settings():
    return rs.ResampleSettings(struct_size=C.sizeof(rs.ResampleSettings), width=W, height=H, factor=F, pick_mode=0, phase=1,
                               sigma_normal_pow2=2.0, sigma_plane=0.05)


RAYS7 = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")
REPROJECT_PLANES = ("color", "position", "normal", "ids", "variance_in", "prev_position", "prev_normal", "prev_ids", "hist_color",
                    "hist_moments", "out", "moments_out", "variance_out")
UPSAMPLE_ORDER = ("position", "normal", "position_lo", "normal_lo", "picks", "color_lo", "out")


def _downsample(p):
    src, dst = rs.pointer_array([p["src0"], p["src1"]]), rs.pointer_array([p["dst0"], p["dst1"]])
    return rs.lib().mpr_downsample(NO_DEVICE, C.byref(_resample_settings()), p["position"], p["normal"], 2, src, dst, p["picks"], None)


# entry point -> (wrapper module, planes (16 bytes), word arrays (4 bytes), what else the call takes a buffer for, the call).
# The nullable planes are all passed, so each is read by the check.
ENTRIES = {
    "mpl_generate": (ll, ("position", "normal"), RAYS7 + ("weight",), (),
                     lambda p: ll.lib().mpl_generate(NO_DEVICE, C.byref(_lights_settings()), _TABLE, p["position"], p["normal"],
                                                     *[p[k] for k in RAYS7], p["weight"], None)),
    "mpl_resolve": (ll, ("sums", "out"), ("tmax", "weight"), ("occluded",),
                    lambda p: ll.lib().mpl_resolve(NO_DEVICE, C.byref(_lights_settings()), _TABLE, p["tmax"], p["weight"], p["occluded"],
                                                   p["sums"], p["out"], None)),
    "mps_generate": (sv, ("position", "normal"), RAYS7, (),
                     lambda p: sv.lib().mps_generate(NO_DEVICE, C.byref(_secondary_settings()), p["position"], p["normal"],
                                                     *[p[k] for k in RAYS7], None)),
    "mps_resolve": (sv, ("counts", "out"), ("tmax",), ("occluded",),
                    lambda p: sv.lib().mps_resolve(NO_DEVICE, C.byref(_secondary_settings()), p["tmax"], p["occluded"], p["counts"], p["out"],
                                                   None)),
    "mpd_atrous": (dn, ("color", "normal_depth", "albedo", "variance", "scratch", "out", "variance_out"), (), (),
                   lambda p: dn.lib().mpd_atrous(NO_DEVICE, C.byref(_denoise_settings()), p["color"], p["normal_depth"], p["albedo"],
                                                 p["variance"], p["scratch"], p["out"], p["variance_out"], None)),
    "mpd_variance_from_moments": (dn, ("shade", "shade_sq", "variance"), (), (),
                                  lambda p: dn.lib().mpd_variance_from_moments(NO_DEVICE, W, H, 8, p["shade"], p["shade_sq"], p["variance"],
                                                                               None)),
    "mpa_tile_error": (ad, ("shade", "shade_sq"), (), ("wh", "open", "max_err"),
                       lambda p: ad.lib().mpa_tile_error(NO_DEVICE, TS, SLOTS, 16, 0.1, 0.05, p["shade"], p["shade_sq"], p["wh"], p["open"],
                                                         p["max_err"], None)),
    "mpa_move_tiles": (ad, ("src", "dst"), (), ("src_slot", "dst_slot"),
                       lambda p: ad.lib().mpa_move_tiles(NO_DEVICE, TS, SLOTS, p["src"], SLOTS, p["src_slot"], p["dst"], SLOTS,
                                                         p["dst_slot"], None)),
    "mpa_finish_tiles": (ad, ("plane",), (), ("samples", "wh"),
                         lambda p: ad.lib().mpa_finish_tiles(NO_DEVICE, TS, SLOTS, 64, p["plane"], p["samples"], p["wh"], None)),
    "mpt_reproject": (tp, REPROJECT_PLANES, (), (),
                      lambda p: tp.lib().mpt_reproject(NO_DEVICE, C.byref(_temporal_settings()), C.byref(tp.TemporalView()),
                                                       *[p[k] for k in REPROJECT_PLANES], None)),
    "mpt_reset": (tp, ("color", "position", "out", "moments_out"), (), (),
                  lambda p: tp.lib().mpt_reset(NO_DEVICE, W, H, p["color"], p["position"], p["out"], p["moments_out"], None)),
    "mpr_downsample": (rs, ("position", "normal", "src0", "src1", "dst0", "dst1"), ("picks",), (), _downsample),
    "mpr_upsample": (rs, ("position", "normal", "position_lo", "normal_lo", "color_lo", "out"), ("picks",), (),
                     lambda p: rs.lib().mpr_upsample(NO_DEVICE, C.byref(_resample_settings()), *[p[k] for k in UPSAMPLE_ORDER], None)),
}


def _call(entry, moved=None, by=0):
    """(status, message) of `entry` with every buffer on a 16-byte boundary, but `moved` `by` bytes past its own; asserts that
    nothing was launched and nothing written"""
    mod, planes, words, others, call = ENTRIES[entry]
    names = planes + words + others
    arena = np.full((len(names) * REGION + 16) // 4, SENTINEL, np.uint32)
    base = (arena.ctypes.data + 15) & ~15
    ptr = {k: base + i * REGION for i, k in enumerate(names)}
    assert all(v % 16 == 0 for v in ptr.values())
    if moved is not None:
        ptr[moved] += by
    before = mod.last_kernels()
    rc = call(ptr)
    prefix = entry.split("_")[0]
    message = getattr(mod.lib(), f"{prefix}_last_error")().decode()
    assert mod.last_kernels() == before  # mpX_last_kernels is unchanged: nothing was launched
    assert np.all(arena == SENTINEL)     # nothing was written (host memory here: a launch would not even get this far)
    return rc, message


def test_every_buffer_taking_entry_point_is_listed():
    """the table above against the wrappers' signatures: every function of the six libraries that takes a stream takes buffers"""
    listed = set(ENTRIES)
    for mod in (ll, sv, dn, ad, tp, rs):
        for name, (_, args) in mod.SIGNATURES.items():
            takes_buffers = len(args) >= 6  # a device, settings or sizes, buffers and a stream
            assert (name in listed) == takes_buffers, name
    assert len(listed) == 13


@pytest.mark.parametrize("entry", ENTRIES)
def test_aligned_pointers_are_not_refused_for_alignment(entry):
    """nothing wrong: the call gets as far as the device, which does not exist"""
    rc, message = _call(entry)
    assert rc == MP_ERR_HIP and "aligned" not in message, message


PLANE_ARGS = [(e, k) for e, spec in ENTRIES.items() for k in spec[1]]
WORD_ARGS = [(e, k) for e, spec in ENTRIES.items() for k in spec[2]]


@pytest.mark.parametrize("entry,arg", PLANE_ARGS, ids=[f"{e}-{k}" for e, k in PLANE_ARGS])
def test_a_misaligned_plane_is_refused(entry, arg):
    for by in (4, 8, 12):
        rc, message = _call(entry, arg, by)
        assert rc == MP_ERR_INVALID and message == "a plane is not 16-byte aligned", (by, rc, message)


@pytest.mark.parametrize("entry,arg", WORD_ARGS, ids=[f"{e}-{k}" for e, k in WORD_ARGS])
def test_a_misaligned_word_array_is_refused_and_an_odd_word_is_not(entry, arg):
    """ray arrays and picks: 1, 2 or 3 bytes past a word are refused; 4, 8 and 12 bytes past a 16-byte boundary are what the
    headers allow"""
    for by in (1, 2, 3, 5, 7):
        rc, message = _call(entry, arg, by)
        assert rc == MP_ERR_INVALID and message.endswith("is not 4-byte aligned"), (by, rc, message)
    for by in (4, 8, 12):
        rc, message = _call(entry, arg, by)
        assert rc == MP_ERR_HIP and "aligned" not in message, (by, rc, message)


@pytest.mark.parametrize("entry", ["mpl_resolve", "mps_resolve"])
def test_occluded_has_no_rule(entry):
    for by in (1, 2, 3):
        rc, message = _call(entry, "occluded", by)
        assert rc == MP_ERR_HIP and "aligned" not in message, (by, rc, message)


def test_the_earlier_refusals_come_first():
    """a NULL argument and an overlap keep their messages when a plane of the call is misaligned too"""
    st = _lights_settings()
    arena = np.full(4096, SENTINEL, np.uint32)
    base = (arena.ctypes.data + 15) & ~15
    tmax, weight, occluded = base, base + 1024, base + 2048
    sums = base + 4096
    L = ll.lib()
    assert L.mpl_resolve(NO_DEVICE, C.byref(st), _TABLE, tmax, weight, None, sums + 4, None, None) == MP_ERR_INVALID
    assert L.mpl_last_error() == b"NULL argument"
    assert L.mpl_resolve(NO_DEVICE, C.byref(st), _TABLE, tmax, weight, occluded, weight + 4, None, None) == MP_ERR_INVALID
    assert L.mpl_last_error() == b"an output overlaps another buffer of the call"
    assert L.mpl_resolve(NO_DEVICE, C.byref(st), _TABLE, tmax, weight, occluded, sums + 4, None, None) == MP_ERR_INVALID
    assert L.mpl_last_error() == b"a plane is not 16-byte aligned"
    assert np.all(arena == SENTINEL)


# ---- the wrappers' check ----------------------------------------------------------------------------------------------------------
class _OnGpu(torch.Tensor):
    """a CPU tensor that says it lives on cuda:0: expect_plane reads is_cuda, device, dtype, shape, is_contiguous() and data_ptr()"""

    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 0))


def _view(skip_floats, shape=(3, 5, 4)):
    n = shape[0] * shape[1] * shape[2]
    whole = torch.zeros(n + skip_floats + 8, dtype=torch.float32)
    lead = (-whole.data_ptr() % 16) // 4  # floats to the first 16-byte boundary
    return whole[lead + skip_floats:lead + skip_floats + n].view(shape).as_subclass(_OnGpu)


def test_expect_plane_takes_aligned_views():
    for skip in (0, 4, 1024 + 4):  # a fresh tensor; views 16 and 4096 + 16 bytes into a larger one
        t = _view(skip)
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        assert _postlib.expect_plane(t, "color", torch.device("cuda", 0), 0, (3, 5, 4)) is t


@pytest.mark.parametrize("skip", [1, 2, 3, 5])
def test_expect_plane_refuses_a_misaligned_view(skip):
    """whole[1:1 + n].view(h, w, 4) is contiguous and starts 4 bytes off"""
    t = _view(skip)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * (skip % 4)
    with pytest.raises(ValueError) as e:
        _postlib.expect_plane(t, "color", torch.device("cuda", 0), 0, (3, 5, 4))
    text = str(e.value)
    assert text.startswith("color: a contiguous, 16-byte aligned float32 [3, 5, 4] tensor on cuda:0 is expected") and f"{4 * (skip % 4)} bytes" in text


def test_expect_plane_reports_the_other_faults_as_before():
    """a misaligned tensor of a wrong shape gets the usual text: the alignment is asked of what is otherwise a plane"""
    t = _view(1, shape=(5, 3, 4))
    with pytest.raises(ValueError) as e:
        _postlib.expect_plane(t, "color", torch.device("cuda", 0), 0, (3, 5, 4))
    assert str(e.value) == "color: a contiguous float32 [3, 5, 4] tensor on cuda:0 is expected"


@pytest.mark.parametrize("cls,attrs", [(dn.AtrousDenoiser, {}), (tp.TemporalAccumulator, {}), (sv.SecondaryVisibility, {}),
                                       (rs.GuidedResampler, dict(low_resolution=(3, 2))), (ll.LocalLights, {})],
                         ids=lambda v: getattr(v, "__name__", ""))
def test_every_wrapper_checks_its_planes_through_expect_plane(cls, attrs):
    o = object.__new__(cls)
    o.device, o.device_id, o.width, o.height = torch.device("cuda", 0), 0, 5, 3
    for k, v in attrs.items():
        setattr(o, k, v)
    assert o._plane(_view(4), "position").data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="16-byte aligned"):
        o._plane(_view(1), "position")
