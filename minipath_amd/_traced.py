"""What the stages that trace through mp_occluded_rays (SecondaryVisibility, LocalLights, SkyLight) share: the checks of a scene
and its device, the SoA ray buffers, and the loop that runs a call's samples in batches of  generate -> mp_occluded_rays -> resolve.
"""
from __future__ import annotations

from . import _lib as _hip
from ._lib import MinipathError
from ._postlib import Stage

TRACED_ARRAYS = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")  # what mp_occluded_rays takes


class TracedStage(Stage):
    """A Stage for one scene: it owns the ray buffers of `batch` samples per pixel and its result planes.  A subclass names the
    ray arrays its generate step writes (`ray_arrays`, TRACED_ARRAYS first), its [h, w, 4] float32 planes (`planes`) and the
    limit of a call's samples (`max_samples`, its library's own constant)."""

    ray_arrays = TRACED_ARRAYS
    planes = ()
    max_samples = 0

    def __init__(self, scene, resolution, device, batch):
        obj = getattr(scene, "object", scene)
        if obj.ctx is None:
            raise MinipathError(1, "host-only BVH cannot be traced: pass a Context to with_obj/build")
        if device is None:
            device = obj.ctx.device_id
        super().__init__(resolution, device)
        if self.device_id != obj.ctx.device_id:
            raise ValueError(f"the scene lives on device {obj.ctx.device_id}, not {self.device_id}")
        self.scene, self.object = scene, obj
        self.batch = int(batch)
        self._buffers, self._rays = None, 0  # made on first use

    @staticmethod
    def eye_of(camera):
        """The `eye` of a Camera: its lens centre, the first of Camera.center_forward_up_right() (what TemporalAccumulator.view_of
        calls `center`)."""
        return [float(v) for v in camera.center_forward_up_right()[0]]

    def _samples(self, samples) -> int:
        samples = int(samples)
        if not 0 < samples <= self.max_samples:
            raise ValueError(f"samples: 1 .. {self.max_samples} is expected")
        return samples

    def buffers(self, rays_per_sample: int = 1) -> dict:
        """The buffers by name: the `ray_arrays` and "occluded" for width * height * batch * rays_per_sample rays, and the
        `planes`.  Made on first use; a call that needs more rays than any before (LocalLights with more lights) gets new ray
        buffers and keeps the planes."""
        import torch

        n = self.width * self.height * self.batch * rays_per_sample
        if self._buffers is None or self._rays < n:
            old = self._buffers or {}
            b = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k in self.ray_arrays}
            b["occluded"] = torch.empty(n, dtype=torch.uint8, device=self.device)
            for k in self.planes:
                b[k] = old[k] if k in old else torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self.device)
            self._buffers, self._rays = b, n
        return self._buffers

    def _trace(self, samples: int, rays_per_sample: int, settings, generate, *resolves):
        """`samples` samples in ceil(samples / batch) batches on the current torch stream, without a host synchronisation.  Per
        batch: st = settings(begin, n) for its samples [begin, begin + n) -- the stage's settings, accumulating iff begin != 0 --
        then generate(st, b, stream), mp_occluded_rays on the width * height * n * rays_per_sample rays it wrote, and each of
        resolves(st, b, last, stream); b = buffers(rays_per_sample), which is returned; `last` is true in the last batch, the only
        one that writes a resolve's `out`."""
        b = self.buffers(rays_per_sample)
        rays = [b[k].data_ptr() for k in TRACED_ARRAYS]
        stream = self._stream()
        hip, ctx = _hip.lib(), self.object.ctx
        for begin in range(0, samples, self.batch):
            n = min(self.batch, samples - begin)
            st = settings(begin, n)
            generate(st, b, stream)
            # the SoA buffers as they are: no transposes, each ray with its own tmax, and rays with tmax <= 0 are not walked
            _hip.check(hip.mp_occluded_rays(ctx.handle, self.object.handle, *rays, self.width * self.height * n * rays_per_sample,
                                            b["occluded"].data_ptr(), stream))
            for resolve in resolves:
                resolve(st, b, begin + n == samples, stream)
        return b
