"""include/hr_probe_vis.h without a GPU: the exported surface and its Python mirror, the struct sizes, every refusal as a status code (no context,
no device), the C++ members of hr::DeferredShading, and the proof that moving gb_pixel_dir into csrc/pixel_dir.h left k_gbuffer_raycast's code alone."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import probe_vis_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


@pytest.fixture(scope="module")
def pv():
    from hybrid_rendering_amd import build as hb, probe_vis
    hb.build()
    return probe_vis


def test_header_symbols_are_exported_and_mirrored(pv):
    text = open(os.path.join(ROOT, "include", "hr_probe_vis.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hr_[a-z0-9_]+)\s*\(", text)))
    assert decl == ["hr_deferred_render_probes", "hr_probe_vis_default_params", "hr_probe_vis_render"]
    L = pv.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(pv.ABI_SYMBOLS) == decl
    from hybrid_rendering_amd import api, api_deferred, env, env_sources
    for other in (api.ABI_SYMBOLS, env.ABI_SYMBOLS, env_sources.ABI_SYMBOLS):
        assert not set(pv.ABI_SYMBOLS) & set(other)
    assert '#include "hr_api.h"' in text and 'extern "C"' in text
    assert hasattr(api_deferred.DeferredShading, "render_probes")
    assert L.hr_api_revision() == 6
    assert "hr_probe_vis.h" in open(os.path.join(ROOT, "docs", "API_HISTORY.md")).read()


def test_struct_sizes_and_defaults(pv):
    from hybrid_rendering_amd import api, api_gi
    assert C.sizeof(pv.hr_probe_vis_params) == 8 and C.sizeof(api_gi.hr_ddgi_uniforms) == 88 and C.sizeof(api.hr_ubo) == 416 and C.sizeof(api.hr_image_view) == 24
    p = pv.default_params()
    assert (p.radius, p.what) == (0.5, 0)
    pv.lib().hr_probe_vis_default_params(None)     # NULL: nothing happens
    q = pv.params(radius=2.5, what=1)
    assert (q.radius, q.what) == (2.5, 1)


class _Call:
    """hr_probe_vis_render over host stand-ins: the pointers are never followed before the context is looked at, and the context is NULL"""

    def __init__(self, pv):
        from hybrid_rendering_amd import api, api_gi
        self.pv, self.api = pv, api
        b = pc.build("outside_near_r1")
        self.ubo, self.grid = api.make_ubo(b["ubo"]), api_gi.make_uniforms(b["grid"])
        g = self.grid
        self.buf = (C.c_float * 4)()
        ptr = C.cast(self.buf, C.c_void_p)
        self.irr = api.hr_image_view(ptr, g.irradiance_texture_width, g.irradiance_texture_height, g.irradiance_texture_width * 8, 4)
        self.dep = api.hr_image_view(ptr, g.depth_texture_width, g.depth_texture_height, g.depth_texture_width * 4, 3)
        self.color = api.hr_image_view(ptr, 96, 54, 96 * 8, 4)
        self.params = pv.default_params()

    def __call__(self, **kw):
        """kw replaces an argument: None for NULL"""
        a = dict(ubo=self.ubo, grid=self.grid, irr=self.irr, dep=self.dep, params=self.params, depth_in=self.buf, color=self.color)
        a.update(kw)
        ref = lambda v: C.byref(v) if v is not None else None
        L = self.pv.lib()
        st = L.hr_probe_vis_render(None, ref(a["ubo"]), ref(a["grid"]), ref(a["irr"]), ref(a["dep"]), ref(a["params"]), a["depth_in"], ref(a["color"]), None, None, None)
        return st, L.hr_last_error()


def _copy(s, **fields):
    c = type(s).from_buffer_copy(s)
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def test_refusals_are_status_codes_before_the_context_is_needed(pv):
    call = _Call(pv)
    # a good call ends at the NULL context, also without the optional atlas
    assert call() == (INVALID_ARG, b"hr_probe_vis_render: ctx is NULL")
    assert call(dep=None) == (INVALID_ARG, b"hr_probe_vis_render: ctx is NULL")
    assert call(params=pv.params(what=1))[1].endswith(b"ctx is NULL")
    bad = []
    for arg, word in (("ubo", b"ubo is NULL"), ("grid", b"grid is NULL"), ("irr", b"irradiance is NULL"), ("params", b"params is NULL"), ("depth_in", b"depth_in is NULL"),
                      ("color", b"color is NULL")):
        bad.append((dict([(arg, None)]), word))
    bad.append((dict(irr=_copy(call.irr, data=None)), b"irradiance is NULL"))
    bad.append((dict(color=_copy(call.color, data=None)), b"color is NULL"))
    for r in (0.0, -0.5, -0.0, math.inf, -math.inf, math.nan):
        bad.append((dict(params=pv.params(radius=r)), b"radius"))
    for w in (-1, 2, 2 ** 31 - 1):
        bad.append((dict(params=pv.params(what=w)), b"what outside"))
    bad.append((dict(params=pv.params(what=1), dep=None), b"needs the depth atlas"))
    bad.append((dict(params=pv.params(what=1), dep=_copy(call.dep, data=None)), b"needs the depth atlas"))
    for axis in range(3):
        for n in (0, -1):
            bad.append((dict(grid=_copy(call.grid, probe_counts=(axis, n))), b"probe_counts below 1"))
    bad.append((dict(grid=_copy(call.grid, probe_counts=(0, 5))), b"irradiance atlas extents disagree"))               # the atlas is another grid's
    bad.append((dict(grid=_copy(call.grid, irradiance_texture_width=call.grid.irradiance_texture_width + 1)), b"irradiance atlas extents disagree"))
    bad.append((dict(grid=_copy(call.grid, irradiance_probe_side_length=0)), b"irradiance atlas extents disagree"))
    bad.append((dict(irr=_copy(call.irr, width=call.irr.width - 1)), b"irradiance view disagrees"))
    bad.append((dict(irr=_copy(call.irr, height=call.irr.height + 10)), b"irradiance view disagrees"))
    bad.append((dict(irr=_copy(call.irr, format=3)), b"irradiance view disagrees"))
    bad.append((dict(params=pv.params(what=1), dep=_copy(call.dep, format=4)), b"depth atlas view disagrees"))
    bad.append((dict(params=pv.params(what=1), dep=_copy(call.dep, width=call.dep.width + 18)), b"depth atlas view disagrees"))
    bad.append((dict(params=pv.params(what=1), grid=_copy(call.grid, depth_texture_height=7)), b"depth atlas extents disagree"))
    for fmt in (1, 2, 3, 5, 6):
        bad.append((dict(color=_copy(call.color, format=fmt)), b"color is not RGBA16F"))
    bad.append((dict(color=_copy(call.color, width=0)), b"color extent"))
    assert len(bad) > 35
    for kw, word in bad:
        st, msg = call(**kw)
        assert st == INVALID_ARG and word in msg and msg.startswith(b"hr_probe_vis_render: ") and b"ctx is NULL" not in msg, (kw, msg)
    # a depth atlas that disagrees is not looked at when what == 0
    assert call(dep=_copy(call.dep, format=4))[1].endswith(b"ctx is NULL")
    L = pv.lib()
    p = pv.default_params()
    assert L.hr_deferred_render_probes(None, None, None, C.byref(p), None, None, None) == INVALID_ARG and L.hr_last_error() == b"hr_deferred_render_probes: deferred is NULL"


def test_deferred_shading_members_compile():
    """include/hr/passes.hpp: the four members of the reference's class, and render() with the trailing DDGI*"""
    code = ('#include <hr/passes.hpp>\n'
            'float members(hr::DeferredShading& d) { d.set_visualize_probe_grid(true); d.set_probe_visualization_scale(0.5f);\n'
            '  return d.visualize_probe_grid() ? d.probe_visualization_scale() : 0.0f; }\n'
            'void frame(hr::DeferredShading& d, hr::Stream s, const hr::Frame& f, const hr::ImageView* v, hr::DDGI* ddgi, hr::RayTracedAO* ao, hr::RayTracedShadows* sh,\n'
            '           hr::RayTracedReflections* re) { d.render(s, f, v, v, v, v); d.render(s, f, v, v, v, v, ddgi); d.render(s, ao, sh, re, ddgi); }\n'
            'int main() { static_assert(sizeof(hr_probe_vis_params) == 8, "hr_probe_vis_params"); hr_probe_vis_params p; hr_probe_vis_default_params(&p); return p.what; }\n')
    with tempfile.NamedTemporaryFile("w", suffix=".cpp", delete=False) as f:
        f.write(code)
    try:
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), f.name])
    finally:
        os.unlink(f.name)


# tools/isa_stats.py's hash of every k_gbuffer_raycast instantiation before gb_pixel_dir moved into csrc/pixel_dir.h
GBUFFER_ISA = {"<false, false, false>": "972e5df12c", "<false, false, true>": "6a75d44228", "<false, true, false>": "69da2ca3b5", "<false, true, true>": "9fcf0896bf",
               "<true, false, false>": "1673dc18bd", "<true, false, true>": "6d1d8b75c4", "<true, true, false>": "2507d7a122", "<true, true, true>": "815c010985"}


def test_moving_gb_pixel_dir_left_the_gbuffer_kernels_alone():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), os.path.join(ROOT, "hybrid_rendering_amd", "csrc", "api.hip"), "k_gbuffer_raycast"],
                         capture_output=True, text=True, check=True).stdout
    got = dict(re.findall(r"k_gbuffer_raycast(<[a-z, ]+>)\s+isa ([0-9a-f]{10})", out))
    assert got == GBUFFER_ISA, out
    api_hip = open(os.path.join(ROOT, "hybrid_rendering_amd", "csrc", "api.hip")).read()
    assert "gb_pixel_dir(const" not in api_hip and '#include "pixel_dir.h"' in api_hip
