"""`Renderer` (reference src/renderer.rs:18-115): the builder and the two public entry
points.  `sample()` — the seam of SURVEY §8b — is one call into the C ABI
(`rptgpu_render_batch`); nothing of the path tracer is computed in Python."""
import math

from . import _abi
from .buffer import Buffer, Filter
from .device import DeviceBuffer, GpuScene, make_params


class Renderer:
    def __init__(self, scene, camera):  # Renderer::new, renderer.rs:46-57
        self.scene = scene
        self.camera = camera
        self._width = 800
        self._height = 600
        self._exposure_value = 0.0
        self._filter = Filter()
        self._max_bounces = 0
        self._num_samples = 1
        # additions (the reference has no seed and no device): see include/rpt_gpu.h
        self._seed = 0x52505447
        self._device = 0
        self._precision = _abi.RPT_PRECISION_F64_STRICT
        self._samples_done = 0
        self._gpu = None

    def width(self, width):  # renderer.rs:60-63
        self._width = int(width)
        return self

    def height(self, height):  # renderer.rs:66-69
        self._height = int(height)
        return self

    def exposure_value(self, ev):  # renderer.rs:72-75
        self._exposure_value = float(ev)
        return self

    def filter(self, filter):  # renderer.rs:78-81
        self._filter = filter
        return self

    def max_bounces(self, n):  # renderer.rs:84-87
        self._max_bounces = int(n)
        return self

    def num_samples(self, n):  # renderer.rs:90-93
        self._num_samples = int(n)
        return self

    def seed(self, seed):
        self._seed = int(seed)
        return self

    def device(self, device):
        self._device = int(device)
        return self

    def precision(self, mode):
        self._precision = int(mode)
        return self

    def with_gpu_scene(self, gpu_scene):
        """Render with an existing GpuScene (for example one kept across the frames of an animation and moved with
        GpuScene.update) instead of creating one from `scene`."""
        self._gpu = gpu_scene
        self._device = gpu_scene.device
        return self

    def gpu_scene(self):
        if self._gpu is None:
            self._gpu = GpuScene(self.scene, self._device)
        return self._gpu

    def render(self):  # renderer.rs:96-100 -> (H, W, 3) uint8
        buffer = Buffer(self._width, self._height, self._filter)
        self._samples_done = 0
        self.sample(self._num_samples, buffer)
        return buffer.image()

    def iterative_render(self, callback_interval, callback, on_device=False):  # renderer.rs:103-115
        """`on_device=True` keeps the Buffer on the GPU (rptgpu_buffer_*): the callback receives a
        DeviceBuffer with the same image() / variance() and no batch ever travels to the host."""
        if on_device:
            buffer = DeviceBuffer(self.gpu_scene(), self._width, self._height, self._filter)
            iteration = 0
            self._samples_done = 0
            while iteration < self._num_samples:
                steps = min(self._num_samples - iteration, int(callback_interval))
                params = make_params(self._width, self._height, self._max_bounces, steps, self._exposure_value,
                                     self._seed, self._samples_done, precision=self._precision)
                buffer.sample(self.camera, params)
                self._samples_done += steps
                iteration += steps
                callback(iteration, buffer)
            buffer.close()
            return
        buffer = Buffer(self._width, self._height, self._filter)
        iteration = 0
        self._samples_done = 0
        while iteration < self._num_samples:
            steps = min(self._num_samples - iteration, int(callback_interval))
            self.sample(steps, buffer)
            iteration += steps
            callback(iteration, buffer)

    def adaptive_render(self, callback_interval, callback=None, min_batches=4, abs_tol=0.0, rel_tol=0.01):
        """iterative_render(on_device=True) that stops sampling converged pixels (DeviceBuffer.sample_adaptive): rounds
        of callback_interval samples until no pixel is active or num_samples samples per pixel have run;
        callback(iteration, buffer, active) after each round.  -> the (H, W, 3) uint8 image."""
        buffer = DeviceBuffer(self.gpu_scene(), self._width, self._height, self._filter)
        try:
            iteration = 0
            active = self._width * self._height
            self._samples_done = 0
            while iteration < self._num_samples and active:
                steps = min(self._num_samples - iteration, int(callback_interval))
                params = make_params(self._width, self._height, self._max_bounces, steps, self._exposure_value,
                                     self._seed, self._samples_done, precision=self._precision)
                active = buffer.sample_adaptive(self.camera, params, min_batches, abs_tol, rel_tol)
                self._samples_done += steps
                iteration += steps
                if callback is not None:
                    callback(iteration, buffer, active)
            return buffer.image()
        finally:
            buffer.close()

    def denoised_render(self, callback_interval, feature_samples=4, **filter):
        """iterative_render(on_device=True) in batches of callback_interval samples — at least two, else ValueError: one
        batch has no variance — then the first-hit features of samples 0 .. feature_samples-1 and the feature-guided
        filter (DeviceBuffer.denoise's keywords in `filter`), all on the device.  -> the (H, W, 3) uint8 image."""
        if int(callback_interval) < 1 or self._num_samples <= int(callback_interval):
            raise ValueError("denoised_render: num_samples must exceed callback_interval (at least two batches)")
        buffer = DeviceBuffer(self.gpu_scene(), self._width, self._height, self._filter)
        try:
            iteration = 0
            self._samples_done = 0
            while iteration < self._num_samples:
                steps = min(self._num_samples - iteration, int(callback_interval))
                params = make_params(self._width, self._height, self._max_bounces, steps, self._exposure_value,
                                     self._seed, self._samples_done, precision=self._precision)
                buffer.sample(self.camera, params)
                self._samples_done += steps
                iteration += steps
            buffer.features(self.camera, make_params(self._width, self._height, self._max_bounces, int(feature_samples),
                                                     self._exposure_value, self._seed, 0, precision=self._precision))
            return buffer.denoised_image(**filter)
        finally:
            buffer.close()

    def render_aovs(self, channels=_abi.RPT_AOV_ALL):
        """The first-hit feature buffers of this renderer's frame (width, height, seed, num_samples camera rays per pixel:
        the rays render() starts its paths with) as MEANS over each pixel's hits: GpuScene.render_aov's dict with `depth`,
        `normal`, `albedo`, `position` divided by `hits`; a pixel without a hit holds 0, never NaN.  `hits` and `object`
        are returned as they are."""
        import numpy as np
        params = make_params(self._width, self._height, self._max_bounces, self._num_samples, self._exposure_value,
                             self._seed, 0, precision=self._precision)
        out = self.gpu_scene().render_aov(self.camera, params, channels)
        hits = out["hits"]
        n = np.where(hits > 0, hits, 1).astype(np.float64)
        for name in ("depth", "normal", "albedo", "position"):
            if name in out:
                mean = out[name] / (n if out[name].ndim == 2 else n[..., None])
                mean[hits == 0] = 0.0
                out[name] = mean
        return out

    def sample(self, iterations, buffer):  # renderer.rs:117-129 — THE hot path, on the GPU
        params = make_params(self._width, self._height, self._max_bounces, iterations,
                             self._exposure_value, self._seed, self._samples_done,
                             precision=self._precision)
        colors = self.gpu_scene().render_batch(self.camera, params)
        self._samples_done += iterations
        buffer.add_samples(colors)
