"""Python mirror of include/hr_probe_vis.h: the DDGI probe-grid visualisation (csrc/probe_vis.hip; the arithmetic is specified in
hr_probe_vis.h).  ``render`` is the stateless call over tensors; ``api_deferred.DeferredShading.render_probes`` draws onto a composite
pass's own output with a DDGI pass's current atlases."""
from __future__ import annotations

import ctypes as C

from .api import _check, _stream_ptr, hr_image_view, lib, make_ubo
from .api_gi import hr_ddgi_uniforms, make_uniforms

# every symbol include/hr_probe_vis.h declares (tests/test_probe_vis_host.py); kept apart from api.ABI_SYMBOLS
ABI_SYMBOLS = ["hr_probe_vis_default_params", "hr_probe_vis_render", "hr_deferred_render_probes"]

WHAT_IRRADIANCE, WHAT_DEPTH = 0, 1


class hr_probe_vis_params(C.Structure):
    _fields_ = [("radius", C.c_float), ("what", C.c_int32)]


def default_params() -> hr_probe_vis_params:
    p = hr_probe_vis_params()
    lib().hr_probe_vis_default_params(C.byref(p))
    return p


def params(radius=None, what=None) -> hr_probe_vis_params:
    """hr_probe_vis_default_params with the given fields replaced"""
    p = default_params()
    if radius is not None:
        p.radius = float(radius)
    if what is not None:
        p.what = int(what)
    return p


def _atlas_view(t, channels):
    """cuda fp16 tensor [H, W, channels], contiguous -> hr_image_view"""
    assert t.dim() == 3 and int(t.shape[2]) == channels and t.element_size() == 2 and t.is_contiguous() and t.is_cuda, f"atlas: cuda float16 [h,w,{channels}]"
    return hr_image_view(C.c_void_p(t.data_ptr()), int(t.shape[1]), int(t.shape[0]), int(t.shape[1]) * 2 * channels, {2: 3, 4: 4}[channels])


def _opt(t, itemsize, shape, name):
    if t is None:
        return None
    assert tuple(t.shape) == tuple(shape) and t.element_size() == itemsize and t.is_contiguous() and t.is_cuda, f"{name}: cuda [h,w], {itemsize}-byte elements"
    return C.c_void_p(t.data_ptr())


def render(ctx, np_ubo, np_ddgi, irradiance, depth_in, color, depth_atlas=None, radius=0.5, what=0, depth_out=None, probe_id_out=None, stream=None):
    """hr_probe_vis_render.  np_ubo / np_ddgi: the 416- and 88-byte blocks (synth.make_ubo, synth_env.ddgi_uniforms) or the ctypes structs;
    irradiance [H, W, 4] and depth_atlas [H, W, 2] cuda float16; depth_in cuda float32 [h, w]; color cuda float16 [h, w, 4], drawn into in place;
    depth_out (float32, may be depth_in) and probe_id_out (int32) [h, w], optional."""
    ubo = np_ubo if isinstance(np_ubo, C.Structure) else make_ubo(np_ubo)
    grid = np_ddgi if isinstance(np_ddgi, hr_ddgi_uniforms) else make_uniforms(np_ddgi)
    cv = _atlas_view(color, 4)
    h, w = int(color.shape[0]), int(color.shape[1])
    iv = _atlas_view(irradiance, 4)
    dv = _atlas_view(depth_atlas, 2) if depth_atlas is not None else None
    p = params(radius, what)
    _check(lib().hr_probe_vis_render(ctx.h, C.byref(ubo), C.byref(grid), C.byref(iv), C.byref(dv) if dv is not None else None, C.byref(p),
                                     _opt(depth_in, 4, (h, w), "depth_in"), C.byref(cv), _opt(depth_out, 4, (h, w), "depth_out"),
                                     _opt(probe_id_out, 4, (h, w), "probe_id_out"), _stream_ptr(stream)), "hr_probe_vis_render")


def render_probes(deferred_handle, inputs, ddgi_handle, radius=0.5, what=0, depth_out=None, probe_id_out=None, stream=None):
    """hr_deferred_render_probes over the passes' handles (api_deferred.DeferredShading.render_probes)"""
    p = params(radius, what)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _check(lib().hr_deferred_render_probes(deferred_handle, C.byref(inputs), ddgi_handle, C.byref(p), ptr(depth_out), ptr(probe_id_out), _stream_ptr(stream)),
           "hr_deferred_render_probes")
