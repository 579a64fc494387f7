"""What the wrappers of the seven post-process libraries (denoise, adaptive, temporal, secondary, resample, lights, sky) share:
PostLibrary, the loader of a library of its own beside libminipath_hip.so with its mpX_last_error and mpX_last_kernels; Stage, the
base of the per-resolution objects (device, size, current stream, plane check); and the checks of a device and a plane themselves.
The stages that trace through mp_occluded_rays share more: _traced.py.
torch is imported where it is used, so ``import minipath_amd`` works without it.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import MP_OK, MinipathError

_HERE = os.path.dirname(os.path.abspath(__file__))
PLANE_ALIGN = 16  # bytes: what the libraries ask of every plane's first byte


class PostLibrary:
    """libminipath_<name>.so, whose symbols start with `prefix` ("mpd"): loaded on first use with restype and argtypes set from
    `signatures` (name -> (restype, argtypes)).  `what` ends the error of a library that has not been built ("the denoiser has no
    CPU fallback"): there is no other compute path.  A wrapper module makes one and binds its lib, check and last_kernels from it."""

    def __init__(self, name: str, prefix: str, signatures: dict, what: str):
        self.name, self.prefix, self.signatures, self.what = name, prefix, signatures, what
        # MINIPATH_<NAME>_SO: experiment builds of the same library (kernel variants under measurement); default = the in-tree build
        self.path = os.environ.get("MINIPATH_" + name.upper() + "_SO") or os.path.join(_HERE, name, f"libminipath_{name}.so")
        self.handle = None

    def load(self) -> C.CDLL:
        """The library.  Fails loudly when it has not been built."""
        if self.handle is None:
            if not os.path.exists(self.path):
                raise ImportError(f"{self.path} is missing: build it with `make -C minipath_amd/csrc` -- {self.what}")
            try:
                import torch  # noqa: F401  (one HIP runtime per process: torch's loads first, as for libminipath_hip.so)
            except ImportError:
                pass
            L = C.CDLL(self.path)
            for name, (res, args) in self.signatures.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            self.handle = L
        return self.handle

    def check(self, rc: int) -> None:
        if rc != MP_OK:
            msg = getattr(self.load(), self.prefix + "_last_error")()
            raise MinipathError(rc, msg.decode() if msg else "")

    def last_kernels(self) -> list:
        """mpX_last_kernels: the kernels of the calling thread's last launching call, distinct names in launch order.  The size is
        asked for first, then a buffer of that size is filled."""
        fn = getattr(self.load(), self.prefix + "_last_kernels")
        need = C.c_size_t()
        self.check(fn(None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        self.check(fn(buf, need.value + 1, None))
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


class Stage:
    """A stage of one library for one resolution (width, height) on one device.  A subclass names its PostLibrary (`library`) and
    the refusal of a device that is no GPU (`runs_on`), and says whether its planes may be None (`none_passes`)."""

    library: PostLibrary = None
    runs_on = ""
    none_passes = False  # denoise and temporal have nullable planes; the others refuse None like any non-tensor

    def __init__(self, resolution, device):
        self.device, self.device_id = resolve_device(device, self.runs_on)
        self.width, self.height = int(resolution[0]), int(resolution[1])

    def _stream(self):
        return stream_of(self.device)

    def _plane(self, t, name, dtypes=None, kinds=None, size=None):
        """`t` as an image-major [h, w, 4] plane of this stage's size (or of `size` = (w, h)): expect_plane"""
        if t is None and self.none_passes:
            return None
        w, h = size or (self.width, self.height)
        return expect_plane(t, name, self.device, self.device_id, (h, w, 4), dtypes, kinds)

    def last_kernels(self) -> list:
        """The kernels the calling thread's last launching call of this stage's library launched (mpX_last_kernels)."""
        return self.library.last_kernels()
