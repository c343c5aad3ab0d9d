"""Python mirror of include/hr_env.h: the environment's derived inputs on the GPU — SH9 irradiance, the GGX-prefiltered chain and the
split-sum BRDF LUT from a sky cubemap in device memory (csrc/env.hip; the arithmetic is specified in hr_env.h / DESIGN.md §3.5)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import api
from .api import _check, _stream_ptr, lib
from .api_gi import hr_environment

# every symbol include/hr_env.h declares (tests/test_env_host.py); kept apart from api.ABI_SYMBOLS, as comm.ABI_SYMBOLS is
ABI_SYMBOLS = ["hr_env_default_desc", "hr_env_create", "hr_env_update", "hr_env_get", "hr_env_sh9_device", "hr_env_read_sh9", "hr_env_sample_table",
               "hr_env_set_profiling", "hr_env_get_stage_times", "hr_env_destroy", "hr_deferred_bind_sh9"]


class hr_env_desc(C.Structure):
    _fields_ = [("sky_size", C.c_int32), ("prefiltered_size", C.c_int32), ("prefiltered_levels", C.c_int32), ("brdf_lut_size", C.c_int32),
                ("n_samples", C.c_int32)]


def default_desc() -> hr_env_desc:
    d = hr_env_desc()
    lib().hr_env_default_desc(C.byref(d))
    return d


def sample_table(n: int) -> np.ndarray:
    """hr_env_sample_table: [n][4] float32 rows (xi1, cos phi, sin phi, 0).  Host only."""
    out = np.zeros((int(n), 4), np.float32)
    _check(lib().hr_env_sample_table(C.c_int32(int(n)), C.c_void_p(out.ctypes.data)), "hr_env_sample_table")
    return out


def _device_tensor(ptr, shape, typestr):
    import torch

    class _W:
        pass

    w = _W()
    w.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)
    return torch.as_tensor(w, device="cuda")


def bind_sh9(deferred, device_ptr):
    """hr_deferred_bind_sh9: the composite `deferred` (api_deferred.DeferredShading) reads SH9 from device memory; None: from its params again"""
    _check(lib().hr_deferred_bind_sh9(deferred.h, C.c_void_p(device_ptr) if device_ptr else None), "hr_deferred_bind_sh9")


class Environment(api._Pass):
    """hr_env: owns the sky, the prefiltered chain, the BRDF LUT and SH9 in device memory.  ``update(sky)`` derives them from a cuda fp16
    tensor [6,S,S,4]; ``get()`` is the hr_environment every pass takes; ``sh9_device()`` is what ``bind_sh9`` hands to the composite."""
    _prefix = "hr_env"

    def __init__(self, ctx, sky_size=None, prefiltered_size=None, prefiltered_levels=None, brdf_lut_size=None, n_samples=None):
        d = default_desc()
        for name, v in (("sky_size", sky_size), ("prefiltered_size", prefiltered_size), ("prefiltered_levels", prefiltered_levels),
                        ("brdf_lut_size", brdf_lut_size), ("n_samples", n_samples)):
            if v is not None:
                setattr(d, name, int(v))
        self.desc = d
        self.h = C.c_void_p()
        _check(lib().hr_env_create(ctx.h, C.byref(d), C.byref(self.h)), "hr_env_create")

    def update(self, sky, stream=None):
        S = self.desc.sky_size
        assert tuple(sky.shape) == (6, S, S, 4) and sky.element_size() == 2 and sky.is_contiguous() and sky.is_cuda, "sky: cuda fp16 [6,S,S,4]"
        _check(lib().hr_env_update(self.h, C.c_void_p(sky.data_ptr()), _stream_ptr(stream)), "hr_env_update")

    def update_equirect(self, image, stream=None):
        """hr_env_update_equirect (include/hr_env_sources.h): the sky from an equirectangular cuda float32 tensor [h,w,4], e.g. assets.load_hdr's"""
        from . import env_sources
        env_sources.update_equirect(self.h, image, stream)

    def update_sky(self, stream=None, **params):
        """hr_env_update_sky: the analytic sky; sun_dir, turbidity, scale, ground_albedo, each defaulting to hr_sky_default_params'"""
        from . import env_sources
        env_sources.update_sky(self.h, stream, **params)

    def get(self) -> hr_environment:
        e = hr_environment()
        _check(lib().hr_env_get(self.h, C.byref(e)), "hr_env_get")
        e._keep = self
        return e

    def sh9_device(self) -> int:
        p = C.c_void_p()
        _check(lib().hr_env_sh9_device(self.h, C.byref(p)), "hr_env_sh9_device")
        return int(p.value)

    def read_sh9(self) -> np.ndarray:
        out = np.zeros((9, 4), np.float32)
        _check(lib().hr_env_read_sh9(self.h, C.c_void_p(out.ctypes.data)), "hr_env_read_sh9")
        return out

    # zero-copy torch views of the env's own storage (valid until close())
    def sky(self):
        e = self.get()
        return _device_tensor(e.sky, (6, e.sky_size, e.sky_size, 4), "<f2")

    def prefiltered(self):
        """the packed chain, [texels][4] fp16"""
        e = self.get()
        n = sum(6 * (e.prefiltered_size >> l) ** 2 for l in range(e.prefiltered_levels))
        return _device_tensor(e.prefiltered, (n, 4), "<f2")

    def brdf_lut(self):
        e = self.get()
        return _device_tensor(e.brdf_lut, (e.brdf_lut_size, e.brdf_lut_size, 2), "<f2")

    def sh9(self):
        return _device_tensor(self.sh9_device(), (9, 4), "<f4")

    def close(self):
        if self.h:
            lib().hr_env_destroy(self.h)
            self.h = C.c_void_p()
