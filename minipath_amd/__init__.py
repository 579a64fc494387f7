"""minipath_amd -- MI355X (gfx950) implementation of bluecube/minipath's per-pixel sampling hot path.

Host-side mirror of the reference's public API (src/lib.rs:8-10): ``render``, ``RenderProgress``,
``RenderSettings``, ``Camera``, ``Scene`` and ``TriangleBvh``, over the C ABI of ``include/minipath_hip.h``.
All compute happens in ``csrc/libminipath_hip.so`` (hand-written HIP kernels); there is no CPU path here.
"""
from ._lib import AovPlanes, AovPlanesEx, MinipathError, MP_NO_PRIM, MP_LINK_NULL, MAX_MATERIALS, SO_PATH  # noqa: F401
from .camera import Camera, CameraSampler  # noqa: F401
from .screen_block import ScreenBlock, tile_ordering  # noqa: F401
from .scene import Context, Instances, ObjectGroup, Scene, Sphere, TriangleBvh  # noqa: F401
from .renderer import (RenderProgress, RenderProgressSnapshot, RenderSettings, render, render_multi, render_tile,  # noqa: F401
                       FrameRenderer, MultiDeviceFrame)
from .denoise import AtrousDenoiser  # noqa: F401  (denoise/libminipath_denoise.so is loaded on first use, not here)
from .adaptive import AdaptiveSampler  # noqa: F401  (adaptive/libminipath_adaptive.so is loaded on first use, not here)
from .temporal import TemporalAccumulator  # noqa: F401  (temporal/libminipath_temporal.so is loaded on first use, not here)
from .secondary import SecondaryVisibility  # noqa: F401  (secondary/libminipath_secondary.so is loaded on first use, not here)
from .resample import GuidedResampler  # noqa: F401  (resample/libminipath_resample.so is loaded on first use, not here)
from .lights import LocalLights  # noqa: F401  (lights/libminipath_lights.so is loaded on first use, not here)
from .sky import SkyLight, gradient_sky  # noqa: F401  (sky/libminipath_sky.so is loaded on first use, not here)

__all__ = [
    "AdaptiveSampler", "AovPlanes", "AovPlanesEx", "AtrousDenoiser", "Camera", "CameraSampler", "Context", "Instances", "FrameRenderer", "GuidedResampler", "LocalLights", "MinipathError", "MultiDeviceFrame", "ObjectGroup", "RenderProgress", "render_multi",
    "RenderProgressSnapshot", "RenderSettings", "Scene", "ScreenBlock", "SecondaryVisibility", "SkyLight", "Sphere", "TemporalAccumulator", "TriangleBvh", "gradient_sky", "render",
    "render_tile", "tile_ordering",
]
