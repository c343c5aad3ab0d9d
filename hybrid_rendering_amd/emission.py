"""Python mirror of include/hr_emission.h: emissive materials (csrc/emission.hip; the arithmetic is specified in hr_emission.h and restated
in tests/emission_reference.py).  The functions take a scene HANDLE; ``api.Scene`` has them as methods (``set_emission``, ``set_emissive``,
``set_emissive_textures``, ``emission``, ``emissive_image``) and ``api_deferred.DeferredShading.add_emissive`` runs the add stage."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import _check, _ptr, _stream_ptr, hr_image_view, lib, make_ubo

# every symbol include/hr_emission.h declares (tests/test_emission_host.py); kept apart from api.ABI_SYMBOLS
ABI_SYMBOLS = ["hr_scene_set_emission", "hr_scene_get_emission", "hr_scene_set_emissive", "hr_scene_set_emissive_device", "hr_scene_set_emissive_textures",
               "hr_scene_emission", "hr_gbuffer_emissive", "hr_deferred_add_emissive"]

ARGTYPES = {
    "hr_scene_set_emission": [C.c_void_p, C.c_int32, C.c_float, C.c_void_p],
    "hr_scene_get_emission": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)],
    "hr_scene_set_emissive": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_set_emissive_device": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_set_emissive_textures": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_emission": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_gbuffer_emissive": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
    "hr_deferred_add_emissive": [C.c_void_p, C.c_void_p, C.c_void_p],
}


def call(name):
    """the library's function with its argument types set"""
    f = getattr(lib(), name)
    f.argtypes = ARGTYPES[name]
    return f


def set_emission(scene_h, enable: bool, scale: float = 1.0, stream=None):
    """hr_scene_set_emission: opt the scene in (off by default); ``scale`` finite and >= 0"""
    _check(call("hr_scene_set_emission")(scene_h, 1 if enable else 0, float(scale), _stream_ptr(stream)), "hr_scene_set_emission")


def get_emission(scene_h):
    """hr_scene_get_emission -> (enabled, scale)"""
    e, s = C.c_int32(0), C.c_float(0.0)
    _check(call("hr_scene_get_emission")(scene_h, C.byref(e), C.byref(s)), "hr_scene_get_emission")
    return bool(e.value), float(s.value)


def set_emissive(scene_h, n_materials: int, rgb, stream=None):
    """hr_scene_set_emissive (``rgb``: host [n_materials, 3]) or, for a cuda float32 tensor, hr_scene_set_emissive_device (capturable, unchecked)"""
    if hasattr(rgb, "is_cuda") and rgb.is_cuda:
        import torch
        assert rgb.dtype == torch.float32 and tuple(rgb.shape) == (n_materials, 3) and rgb.is_contiguous(), f"rgb: contiguous cuda float32 [{n_materials}, 3]"
        _check(call("hr_scene_set_emissive_device")(scene_h, _ptr(rgb), _stream_ptr(stream)), "hr_scene_set_emissive_device")
        return
    c = np.asarray(rgb)
    if c.shape != (n_materials, 3):
        raise ValueError(f"rgb: one colour per material ({n_materials}, 3), got shape {c.shape}")
    c = np.ascontiguousarray(c, np.float32)
    _check(call("hr_scene_set_emissive")(scene_h, C.c_void_p(c.ctypes.data), _stream_ptr(stream)), "hr_scene_set_emissive")


def set_emissive_textures(scene_h, n_materials: int, tex, stream=None):
    """hr_scene_set_emissive_textures: per material an index into the scene's textures, -1 = none"""
    t = np.asarray(tex)
    if t.shape != (n_materials,):
        raise ValueError(f"tex: one index per material ({n_materials}), got shape {t.shape}")
    t = np.ascontiguousarray(t, np.int32)
    _check(call("hr_scene_set_emissive_textures")(scene_h, C.c_void_p(t.ctypes.data), _stream_ptr(stream)), "hr_scene_set_emissive_textures")


def emission(scene_h, prim, tuv, stream=None):
    """hr_scene_emission: E of the hits (``prim`` cuda int32 [n], ``tuv`` cuda float32 [n, 3], as ``Scene.closest_hit`` returns them) -> cuda float32 [n, 3]"""
    import torch
    assert prim.is_cuda and prim.dtype == torch.int32 and prim.dim() == 1, "prim: cuda int32 [n]"
    assert tuv.is_cuda and tuv.dtype == torch.float32 and tuple(tuv.shape) == (prim.shape[0], 3), "tuv: cuda float32 [n, 3]"
    prim, tuv = prim.contiguous(), tuv.contiguous()
    out = torch.zeros((prim.shape[0], 3), dtype=torch.float32, device=prim.device)
    _check(call("hr_scene_emission")(scene_h, prim.shape[0], _ptr(prim), _ptr(tuv), _ptr(out), _stream_ptr(stream)), "hr_scene_emission")
    return out


def emissive_image(scene_h, np_ubo, w: int, h: int, device="cuda", stream=None):
    """hr_gbuffer_emissive: the emissive image of the primary hits, cuda float16 [h, w, 4] ((E, 1) on surfaces, zeros on sky)"""
    import torch
    out = torch.zeros((h, w, 4), dtype=torch.float16, device=device)
    u = np_ubo if isinstance(np_ubo, C.Structure) else make_ubo(np_ubo)
    _check(call("hr_gbuffer_emissive")(scene_h, C.byref(u), w, h, _ptr(out), _stream_ptr(stream)), "hr_gbuffer_emissive")
    return out


def add_emissive(deferred_h, image, stream=None):
    """hr_deferred_add_emissive: ``image`` (cuda float16 [h, w, 4]) added onto the composite pass's output in place"""
    assert image.dim() == 3 and int(image.shape[2]) == 4 and image.element_size() == 2 and image.is_contiguous() and image.is_cuda, "image: contiguous cuda float16 [h, w, 4]"
    v = hr_image_view(C.c_void_p(image.data_ptr()), int(image.shape[1]), int(image.shape[0]), int(image.shape[1]) * 8, 4)
    _check(call("hr_deferred_add_emissive")(deferred_h, C.byref(v), _stream_ptr(stream)), "hr_deferred_add_emissive")
