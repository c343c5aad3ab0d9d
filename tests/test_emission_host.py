"""include/hr_emission.h without a GPU: the exported surface and its Python mirror, every refusal the calls can make before they need a device as a
status code (never an exception), and the C++ shim."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, 1


@pytest.fixture(scope="module")
def em():
    from hybrid_rendering_amd import build as hb, emission
    hb.build()
    return emission


def test_header_symbols_are_exported_and_mirrored(em):
    text = open(os.path.join(ROOT, "include", "hr_emission.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hr_[a-z0-9_]+)\s*\(", text)))
    assert decl == sorted(["hr_scene_set_emission", "hr_scene_get_emission", "hr_scene_set_emissive", "hr_scene_set_emissive_device", "hr_scene_set_emissive_textures",
                           "hr_scene_emission", "hr_gbuffer_emissive", "hr_deferred_add_emissive"])
    L = em.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(em.ABI_SYMBOLS) == decl and sorted(em.ARGTYPES) == decl
    from hybrid_rendering_amd import api, api_deferred, env, env_sources, probe_vis, skinning
    for other in (api.ABI_SYMBOLS, env.ABI_SYMBOLS, env_sources.ABI_SYMBOLS, probe_vis.ABI_SYMBOLS, skinning.ABI_SYMBOLS):
        assert not set(em.ABI_SYMBOLS) & set(other)
    assert '#include "hr_api.h"' in text and 'extern "C"' in text
    for m in ("set_emission", "set_emissive", "set_emissive_textures", "emission", "emissive_image"):
        assert hasattr(api.Scene, m) and hasattr(api.InstancedScene, m), m
    assert hasattr(api_deferred.DeferredShading, "add_emissive")
    assert "hr_emission.h" in open(os.path.join(ROOT, "docs", "API_HISTORY.md")).read()


def test_refusals_are_status_codes_without_a_scene(em):
    """every call with a NULL scene (or a NULL composite) and with bad arguments: HR_ERR_INVALID_ARG and a message that names the call"""
    L = em.lib()
    buf = (C.c_float * 12)()
    ibuf = (C.c_int32 * 4)()
    en, sc = C.c_int32(7), C.c_float(7.0)
    stub = C.cast(buf, C.c_void_p)              # stands for a scene: the checks below fail before a scene is looked at
    calls = [
        ("hr_scene_set_emission", (None, 1, 1.0, None), b"scene is NULL"),
        ("hr_scene_set_emission", (None, 0, 1.0, None), b"scene is NULL"),
        ("hr_scene_get_emission", (None, C.byref(en), C.byref(sc)), b"scene is NULL"),
        ("hr_scene_set_emissive", (None, buf, None), b"scene is NULL"),
        ("hr_scene_set_emissive_device", (None, buf, None), b"scene is NULL"),
        ("hr_scene_set_emissive_textures", (None, ibuf, None), b"scene is NULL"),
        ("hr_scene_emission", (None, 4, ibuf, buf, buf, None), b"scene is NULL"),
        ("hr_gbuffer_emissive", (None, buf, 4, 4, buf, None), b"scene is NULL"),
        ("hr_deferred_add_emissive", (None, None, None), b"deferred is NULL"),
    ]
    for s in (-1.0, -0.5, math.inf, -math.inf, math.nan):
        calls.append(("hr_scene_set_emission", (stub, 1, s, None), b"scale is not a finite number >= 0"))
        calls.append(("hr_scene_set_emission", (stub, 0, s, None), b"scale is not a finite number >= 0"))
    calls += [
        ("hr_scene_set_emissive", (stub, None, None), b"rgb is NULL"),
        ("hr_scene_set_emissive_device", (stub, None, None), b"rgb is NULL"),
        ("hr_scene_set_emissive_textures", (stub, None, None), b"tex is NULL"),
        ("hr_scene_emission", (stub, -1, ibuf, buf, buf, None), b"n is negative"),
        ("hr_scene_emission", (stub, 4, None, buf, buf, None), b"prim is NULL"),
        ("hr_scene_emission", (stub, 4, ibuf, None, buf, None), b"tuv is NULL"),
        ("hr_scene_emission", (stub, 4, ibuf, buf, None, None), b"out is NULL"),
        ("hr_gbuffer_emissive", (stub, None, 4, 4, buf, None), b"ubo is NULL"),
        ("hr_gbuffer_emissive", (stub, buf, 0, 4, buf, None), b"width or height is not positive"),
        ("hr_gbuffer_emissive", (stub, buf, 4, -3, buf, None), b"width or height is not positive"),
        ("hr_gbuffer_emissive", (stub, buf, 4, 4, None, None), b"out is NULL"),
        ("hr_deferred_add_emissive", (stub, None, None), b"emissive is NULL"),
    ]
    for name, args, word in calls:
        st = em.call(name)(*args)
        msg = L.hr_last_error()
        assert st == INVALID_ARG and word in msg and msg.startswith(name.encode() + b": "), (name, args, st, msg)
    assert (en.value, sc.value) == (7, 7.0), "a refused getter writes nothing"
    # n == 0 asks for nothing: accepted before any pointer is looked at
    assert em.call("hr_scene_emission")(stub, 0, None, None, None, None) == OK
    from hybrid_rendering_amd import api
    v = api.hr_image_view(None, 4, 4, 32, 4)
    assert em.call("hr_deferred_add_emissive")(stub, C.byref(v), None) == INVALID_ARG and L.hr_last_error() == b"hr_deferred_add_emissive: emissive is NULL"


def test_python_wrappers_check_shapes_before_the_library(em):
    with pytest.raises(ValueError, match="one colour per material"):
        em.set_emissive(None, 3, np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="one index per material"):
        em.set_emissive_textures(None, 3, np.zeros(4, np.int32))


def test_the_shims_compile():
    """include/hr/emission.hpp over passes.hpp (C++14), and hr_emission.h alone as C"""
    code = ('#include <hr/emission.hpp>\n'
            'void frame(hr::Scene& s, hr::DeferredShading& d, hr::Stream st, const hr_ubo& ubo, const hr_image_view& v, const float* rgb, const int32_t* tex, void* img,\n'
            '           const int32_t* prim, const float* tuv, float* out) {\n'
            '  hr::set_emission(s, true, 2.0f, st); float sc; bool on = hr::emission_enabled(s, &sc); (void)on;\n'
            '  hr::set_emissive(s, rgb, st); hr::set_emissive_device(s, rgb, st); hr::set_emissive_textures(s, tex, st);\n'
            '  hr::emission(s, 4, prim, tuv, out, st); hr::gbuffer_emissive(s, ubo, 4, 4, img, st); hr::add_emissive(d, v, st); }\n'
            'int main() { return 0; }\n')
    for suffix, text, cmd in ((".cpp", code, ["g++", "-std=c++14"]), (".c", '#include <hr_emission.h>\nint main(void) { return 0; }\n', ["gcc", "-std=c99"])):
        with tempfile.NamedTemporaryFile("w", suffix=suffix, delete=False) as f:
            f.write(text)
        try:
            subprocess.check_call(cmd + ["-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), f.name])
        finally:
            os.unlink(f.name)
