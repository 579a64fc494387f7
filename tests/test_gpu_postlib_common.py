"""GPU test of the launch path the seven post-process libraries share (minipath_amd/post/post_abi.h): a call the runtime refuses
(hipSetDevice on a device that does not exist -- a host-side refusal, nothing is launched) must not make the library's next
launch on the same thread report that refusal as its own.  HIP's last-error state is per thread and sticky, so launch() clears it
before it launches.  Per library: its cheapest launching entry point on 1 x 1 planes, three times -- valid, refused device, valid
again.  The kernels' own results are the business of test_gpu_<library>.py; here the third call only has to give what the first gave.
"""
import ctypes as C

import pytest

from minipath_amd import adaptive, denoise, lights, resample, secondary, sky, temporal

pytestmark = pytest.mark.gpu

MP_OK, MP_ERR_HIP = 0, 4
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _f4(torch, *v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


# Each case: (wrapper module, prefix, kernel the call reports, make(torch) -> (inputs kept alive, call(device_id, out))) where
# `out` is a 16-word int32 tensor pre-filled with the sentinel that the call writes its outputs into.
def _denoise(torch):
    shade, shade_sq = _f4(torch, 2.0, 0.0, 0.0, 1.0), _f4(torch, 5.0, 0.0, 0.0, 1.0)
    return lambda dev, out: denoise.lib().mpd_variance_from_moments(dev, 1, 1, 8, shade.data_ptr(), shade_sq.data_ptr(), out.data_ptr(), None)


def _adaptive(torch):
    src = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device="cuda")  # one tile of one 16-byte pixel
    return lambda dev, out: adaptive.lib().mpa_move_tiles(dev, 1, 1, src.data_ptr(), 1, None, out.data_ptr(), 1, None, None)


def _temporal(torch):
    color, position = _f4(torch, 0.5, 0.25, 0.125, 1.0), _f4(torch, 1.0, 2.0, 3.0, 1.0)
    return lambda dev, out: temporal.lib().mpt_reset(dev, 1, 1, color.data_ptr(), position.data_ptr(), out[0:4].data_ptr(),
                                                     out[4:8].data_ptr(), None)


def _secondary(torch):
    st = secondary.SecondarySettings(C.sizeof(secondary.SecondarySettings), 1, 1, secondary.MPS_MODE_AO, 0, 1, 0, 1, 0)
    st.light[2], st.radius = 1.0, 1.0
    tmax = torch.tensor([1.0], dtype=torch.float32, device="cuda")
    occluded = torch.zeros(1, dtype=torch.uint8, device="cuda")
    return lambda dev, out: secondary.lib().mps_resolve(dev, C.byref(st), tmax.data_ptr(), occluded.data_ptr(), out[0:4].data_ptr(),
                                                        out[4:8].data_ptr(), None)


def _resample(torch):
    st = resample.ResampleSettings(C.sizeof(resample.ResampleSettings), 1, 1, 2, resample.MPR_PICK_PHASE, 0, 1.0, 0.01)
    position, normal = _f4(torch, 1.0, 2.0, 3.0, 1.0), _f4(torch, 0.0, 0.0, 1.0, 4.0)
    return lambda dev, out: resample.lib().mpr_downsample(dev, C.byref(st), position.data_ptr(), normal.data_ptr(), 0, None, None,
                                                          out.data_ptr(), None)


def _lights(torch):
    st = lights.LightsSettings(C.sizeof(lights.LightsSettings), 1, 1, 0, 1, 0, 1, 1, 0)  # one light, one sample, in one batch
    table = lights.light_table([((0.0, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0))])
    tmax = torch.tensor([1.0], dtype=torch.float32, device="cuda")
    weight = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    occluded = torch.zeros(1, dtype=torch.uint8, device="cuda")
    return lambda dev, out: lights.lib().mpl_resolve(dev, C.byref(st), table, tmax.data_ptr(), weight.data_ptr(), occluded.data_ptr(),
                                                     out[0:4].data_ptr(), out[4:8].data_ptr(), None)


def _sky(torch):
    zenith, horizon, ground = ((C.c_float * 3)(*c) for c in ((0.25, 0.5, 1.0), (1.0, 0.75, 0.5), (0.125, 0.0625, 0.03125)))
    return lambda dev, out: sky.lib().mpe_fill_gradient(dev, 1, zenith, horizon, ground, out[0:4].data_ptr(), None)


CASES = {
    "denoise": (denoise, "mpd", "moments_kernel", _denoise),
    "adaptive": (adaptive, "mpa", "move_tiles_kernel", _adaptive),
    "temporal": (temporal, "mpt", "reset_kernel", _temporal),
    "secondary": (secondary, "mps", "resolve_kernel<true>", _secondary),
    "resample": (resample, "mpr", "downsample_kernel<0>", _resample),
    "lights": (lights, "mpl", "irradiance_kernel<true>", _lights),
    "sky": (sky, "mpe", "sky_gradient_kernel", _sky),
}


@pytest.mark.parametrize("name", CASES)
def test_a_refused_device_is_not_blamed_on_the_next_launch(torch, name):
    mod, prefix, kernel, make = CASES[name]
    call = make(torch)
    last_error = getattr(mod.lib(), f"{prefix}_last_error")
    outs = [torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()

    rc = call(0, outs[0])
    assert rc == MP_OK, last_error()
    assert mod.last_kernels() == [kernel]

    rc = call(torch.cuda.device_count(), outs[1])  # no such device: refused by the runtime before anything is launched
    assert rc == MP_ERR_HIP and last_error().startswith(b"hipSetDevice: "), (rc, last_error())
    assert mod.last_kernels() == [kernel]  # a call that launched nothing leaves the record

    rc = call(0, outs[2])
    assert rc == MP_OK, last_error()  # not "<kernel> launch: <the refusal above>"
    assert mod.last_kernels() == [kernel]

    torch.cuda.synchronize()
    first, refused, again = (o.cpu() for o in outs)
    assert bool((refused == SENTINEL).all())
    assert not bool((first == SENTINEL).all()) and torch.equal(again, first)
