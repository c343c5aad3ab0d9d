"""Python mirror of include/hr_lights.h: a per-scene light list in every hit shader, and the primary-surface pass ``Lights`` (csrc/lights.hip;
the arithmetic is specified in hr_lights.h).  The scene functions take a scene HANDLE; ``api.Scene`` has them as methods (``set_lights``,
``set_lights_device``, ``get_lights``) and ``api_deferred.DeferredShading.add_lights`` adds the pass's image after the composite."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import _check, _ptr, _stream_ptr, hr_image_view, lib, view_to_tensor

HR_MAX_LIGHTS = 256

# every symbol include/hr_lights.h declares (tests/test_lights_host.py); kept apart from api.ABI_SYMBOLS
ABI_SYMBOLS = ["hr_scene_set_lights", "hr_scene_set_lights_device", "hr_scene_get_lights", "hr_lights_default_params", "hr_lights_create", "hr_lights_destroy",
               "hr_lights_render", "hr_lights_output"]


class hr_lights_params(C.Structure):
    _fields_ = [("bias", C.c_float)]


ARGTYPES = {
    "hr_scene_set_lights": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p],
    "hr_scene_set_lights_device": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_get_lights": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)],
    "hr_lights_default_params": [C.POINTER(hr_lights_params)],
    "hr_lights_create": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)],
    "hr_lights_destroy": [C.c_void_p],
    "hr_lights_render": [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(hr_lights_params), C.c_void_p],
    "hr_lights_output": [C.c_void_p, C.POINTER(hr_image_view)],
}


def call(name):
    """the library's function with its argument types set"""
    f = getattr(lib(), name)
    f.argtypes = ARGTYPES[name]
    if name == "hr_lights_default_params":
        f.restype = None
    return f


def as_records(lights) -> np.ndarray:
    """``lights`` -> contiguous float32 [n, 4, 4] (hr_light records: rows data0 .. data3).  Accepts [n, 4, 4], [n, 16] or an empty sequence."""
    a = np.asarray(lights, np.float32)
    if a.size == 0:
        return np.zeros((0, 4, 4), np.float32)
    if a.ndim == 2 and a.shape[1] == 16:
        a = a.reshape(-1, 4, 4)
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError(f"lights: hr_light records [n, 4, 4] (or [n, 16]), got shape {a.shape}")
    if a.shape[0] > HR_MAX_LIGHTS:
        raise ValueError(f"lights: at most HR_MAX_LIGHTS ({HR_MAX_LIGHTS}) records, got {a.shape[0]}")
    return np.ascontiguousarray(a)


def light(kind: int, direction=(0.0, 1.0, 0.0), position=(0.0, 0.0, 0.0), colour=(1.0, 1.0, 1.0), intensity=1.0, radius=0.0, cos_outer=0.0, cos_inner=0.0) -> np.ndarray:
    """one hr_light record, float32 [4, 4]: kind 0 directional / 1 point / 2 spot; ``direction`` points TO the light"""
    return np.array([[*direction, intensity], [*position, radius], [*colour, 0.0], [float(kind), cos_outer, cos_inner, 0.0]], np.float32)


def placed_point_lights(lo, hi, n: int, intensity: float = 8.0, seed: int = 7) -> np.ndarray:
    """n deterministic point lights for tools and probes, float32 [n, 4, 4]: spread along the longest axis of the box (lo, hi), at 15 % to 60 % of its
    height, a quarter of the way in from the sides, with seeded pastel colours"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rng = np.random.RandomState(seed)
    long_axis = int(np.argmax((hi - lo) * (1.0, 0.0, 1.0)))
    side = 2 - long_axis
    out = np.zeros((n, 4, 4), np.float32)
    for k in range(n):
        p = np.zeros(3)
        p[long_axis] = lo[long_axis] + (hi - lo)[long_axis] * (k + 0.5) / n
        p[side] = lo[side] + (hi - lo)[side] * (0.25 if k % 2 else 0.75)
        p[1] = lo[1] + (hi - lo)[1] * (0.15 + 0.45 * rng.uniform())
        out[k] = light(1, position=p, colour=0.5 + 0.5 * rng.uniform(size=3), intensity=intensity)
    return out


def set_lights(scene_h, lights, stream=None):
    """hr_scene_set_lights: the scene's list (host records; an empty sequence clears it: off)"""
    a = as_records(lights)
    _check(call("hr_scene_set_lights")(scene_h, C.c_void_p(a.ctypes.data) if a.shape[0] else None, a.shape[0], _stream_ptr(stream)), "hr_scene_set_lights")


def set_lights_device(scene_h, lights, stream=None):
    """hr_scene_set_lights_device: ``lights`` a contiguous cuda float32 tensor of as many records as the last host call set ([n, 4, 4] or [n, 16]);
    one device copy, capturable, unchecked"""
    import torch
    n = get_lights(scene_h).shape[0]
    assert lights.is_cuda and lights.dtype == torch.float32 and lights.is_contiguous() and lights.numel() == n * 16, f"lights: contiguous cuda float32, {n} records of 16 floats"
    _check(call("hr_scene_set_lights_device")(scene_h, _ptr(lights), _stream_ptr(stream)), "hr_scene_set_lights_device")


def get_lights(scene_h) -> np.ndarray:
    """hr_scene_get_lights -> float32 [n, 4, 4], what the host last set"""
    out = np.zeros((HR_MAX_LIGHTS, 4, 4), np.float32)
    n = C.c_int32(0)
    _check(call("hr_scene_get_lights")(scene_h, C.c_void_p(out.ctypes.data), C.byref(n)), "hr_scene_get_lights")
    return out[: n.value].copy()


class Lights:
    """hr_lights: the scene's light list on the primary surfaces, full resolution, hard shadows.  ``render(scene, inputs)`` then ``output()`` (cuda
    float16 [h, w, 4], pass-owned) — add it after the composite with ``DeferredShading.add_lights``."""

    def __init__(self, ctx, width, height):
        self.h = C.c_void_p()
        self.params = hr_lights_params()
        call("hr_lights_default_params")(C.byref(self.params))
        _check(call("hr_lights_create")(ctx.h, width, height, C.byref(self.h)), "hr_lights_create")

    def render(self, scene, inputs, stream=None):
        _check(call("hr_lights_render")(self.h, scene.h, C.addressof(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_lights_render")

    def output(self):
        v = hr_image_view()
        _check(call("hr_lights_output")(self.h, C.byref(v)), "hr_lights_output")
        return view_to_tensor(v)

    def close(self):
        if self.h:
            call("hr_lights_destroy")(self.h)
            self.h = C.c_void_p()
