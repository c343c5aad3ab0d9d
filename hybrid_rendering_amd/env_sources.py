"""Python mirror of include/hr_env_sources.h: what fills an hr_env's sky on the GPU — an equirectangular fp32 map resampled onto the cube, or
the analytic sky (csrc/env_sources.hip; the arithmetic is specified in hr_env_sources.h).  ``env.Environment.update_equirect`` and
``update_sky`` are the object's methods over these calls; ``assets.load_hdr`` reads the Radiance maps ``update_equirect`` takes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import _check, _stream_ptr, lib

# every symbol include/hr_env_sources.h declares (tests/test_env_sources_host.py); kept apart from api.ABI_SYMBOLS and env.ABI_SYMBOLS
ABI_SYMBOLS = ["hr_env_update_equirect", "hr_sky_default_params", "hr_env_update_sky", "hr_env_equirect_table", "hr_sky_coefficients"]


class hr_sky_params(C.Structure):
    _fields_ = [("sun_dir", C.c_float * 3), ("turbidity", C.c_float), ("scale", C.c_float), ("ground_albedo", C.c_float * 3)]


def default_sky_params() -> hr_sky_params:
    p = hr_sky_params()
    lib().hr_sky_default_params(C.byref(p))
    return p


def sky_params(sun_dir=None, turbidity=None, scale=None, ground_albedo=None) -> hr_sky_params:
    """hr_sky_default_params with the given fields replaced"""
    p = default_sky_params()
    if sun_dir is not None:
        p.sun_dir[:] = [float(v) for v in sun_dir]
    if turbidity is not None:
        p.turbidity = float(turbidity)
    if scale is not None:
        p.scale = float(scale)
    if ground_albedo is not None:
        p.ground_albedo[:] = [float(v) for v in ground_albedo]
    return p


def equirect_table(sky_size: int) -> np.ndarray:
    """hr_env_equirect_table: [6][s][s][2] float32 (u, v) of every cube texel.  Host only."""
    s = int(sky_size)
    out = np.zeros((6, max(s, 0), max(s, 0), 2), np.float32)
    _check(lib().hr_env_equirect_table(C.c_int32(s), C.c_void_p(out.ctypes.data)), "hr_env_equirect_table")
    return out


def sky_coefficients(**params) -> np.ndarray:
    """hr_sky_coefficients: the 24 floats the sky kernel takes in its arguments.  Host only."""
    p = sky_params(**params)
    out = np.zeros(24, np.float32)
    _check(lib().hr_sky_coefficients(C.byref(p), C.c_void_p(out.ctypes.data)), "hr_sky_coefficients")
    return out


def update_equirect(env_handle, image, stream=None):
    """hr_env_update_equirect: image = cuda float32 [h, w, 4], contiguous"""
    assert image.dim() == 3 and image.shape[2] == 4 and image.element_size() == 4 and image.is_floating_point() and image.is_contiguous() and image.is_cuda, \
        "equirect image: cuda float32 [h,w,4]"
    _check(lib().hr_env_update_equirect(env_handle, C.c_void_p(image.data_ptr()), C.c_int32(int(image.shape[1])), C.c_int32(int(image.shape[0])), _stream_ptr(stream)),
           "hr_env_update_equirect")


def update_sky(env_handle, stream=None, **params):
    """hr_env_update_sky: sun_dir, turbidity, scale, ground_albedo (each defaults to hr_sky_default_params').  The parameters are read by this call:
    a captured update replays the sky of the capture."""
    p = sky_params(**params)
    _check(lib().hr_env_update_sky(env_handle, C.byref(p), _stream_ptr(stream)), "hr_env_update_sky")
