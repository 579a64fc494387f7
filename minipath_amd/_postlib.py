"""What the wrappers of the post-process libraries (denoise, adaptive, temporal, secondary, resample, lights, sky) share: loading a library
of its own beside libminipath_hip.so, the buffer protocol of its mpX_last_kernels, and the checks of a device and a plane.
torch is imported where it is used, so ``import minipath_amd`` works without it.
"""
from __future__ import annotations

import ctypes as C
import os

PLANE_ALIGN = 16  # bytes: what the libraries ask of every plane's first byte

def load(path: str, signatures: dict, what: str) -> C.CDLL:
    """The library at `path` with restype and argtypes set from `signatures` (name -> (restype, argtypes)).  `what` ends the
    error of a library that has not been built ("the denoiser has no CPU fallback"): there is no other compute path."""
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `make -C minipath_amd/csrc` -- {what}")
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's loads first, as for libminipath_hip.so)
    except ImportError:
        pass
    L = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def last_kernels(fn, check) -> list:
    """The names an mpX_last_kernels `fn` holds: the size is asked for first, then a buffer of that size is filled."""
    need = C.c_size_t()
    check(fn(None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value + 1)
    check(fn(buf, need.value + 1, None))
    return [n for n in buf.value.decode().split("\n") if n]


def resolve_device(device, what: str):
    """(torch.device, device_id) of an index or anything torch.device takes; `what` is the refusal of any other device
    ("the denoiser runs on the GPU")."""
    import torch

    device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if device.type != "cuda":
        raise ValueError(what)
    return device, device.index if device.index is not None else torch.cuda.current_device()


def stream_of(device) -> C.c_void_p:
    """The current torch stream of `device` as the `stream` argument of a call."""
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def expect_plane(t, name: str, device, device_id: int, shape, dtypes=None, kinds=None):
    """`t` if it is a contiguous tensor of `shape` and one of `dtypes` (default: float32) on the device whose first byte is 16-byte
    aligned (the libraries read and write a plane as 16-byte pixels and refuse any other), else ValueError.  A fresh tensor and a
    view that starts a whole number of pixels into one are aligned; a view that starts at an odd float is not.
    `kinds`: how the message names the dtypes, where that is not their names joined by " or "."""
    import torch

    dtypes = dtypes or (torch.float32,)
    kinds = kinds or " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if not (isinstance(t, torch.Tensor) and t.dtype in dtypes and t.is_cuda and t.device.index == device_id
            and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise ValueError(f"{name}: a contiguous {kinds} {list(shape)} tensor on {device} is expected")
    if t.data_ptr() % PLANE_ALIGN:
        raise ValueError(f"{name}: a contiguous, {PLANE_ALIGN}-byte aligned {kinds} {list(shape)} tensor on {device} is expected "
                         f"(this one starts {t.data_ptr() % PLANE_ALIGN} bytes past a {PLANE_ALIGN}-byte boundary)")
    return t
