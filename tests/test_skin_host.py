"""include/hr_skin.h without a GPU: the exported surface, the C++ shim, every refusal of hr_skin_check_desc (a status code, never an exception), and
hr_skin_bounds' own refusals on a host-only skin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skin_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID_ARG, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def sk():
    from hybrid_rendering_amd import build as hb, skinning
    hb.build()
    return skinning


def test_skin_header_symbols_are_exported_and_mirrored(sk):
    text = open(os.path.join(ROOT, "include", "hr_skin.h")).read()
    full = text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hr_[a-z0-9_]+)\s*\(", text)))
    assert len(decl) == 11, decl
    L = sk.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(sk.ABI_SYMBOLS) == decl, set(sk.ABI_SYMBOLS) ^ set(decl)
    from hybrid_rendering_amd import api, env, env_sources
    for other in (api, env, env_sources):
        assert not set(sk.ABI_SYMBOLS) & set(other.ABI_SYMBOLS)
    for h in ("hr_api.h", "hr_api_stages.h", "hr_api_post.h"):
        assert "hr_skin" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert C.sizeof(sk.hr_skin_desc) == 64 and C.sizeof(sk.hr_skin_info_data) == 20
    assert '#include "hr_api.h"' in text and 'extern "C"' in text
    # the contract and what is out of scope stand in the header
    for word in ("Morph.", "Blend.", "Position.", "Normal.", "Tangents are not re-posed", "Dual-quaternion", "More than four influences", "Animation sampling", "indexed variant"):
        assert word in full, word


def test_skin_shim_compiles():
    """include/hr/skinning.hpp is valid C++14 against hr_skin.h and passes.hpp"""
    import subprocess
    import tempfile
    code = ('#include <hr/skinning.hpp>\n'
            'void frame(hr::Scene& scene, hr::Skin& skin, hr::Stream s, const float* pal_dev, const float* pal, const float* mw) {\n'
            '  scene.motion_begin_frame(s); skin.pose(s, pal_dev); skin.pose(s, pal_dev, mw); skin.pose_host(s, pal, mw);\n'
            '  scene.update_vertices(skin.positions(), skin.normals(), 32, skin.n_tris(), s);\n'
            '  float box[6]; hr_mesh_update u = skin.mesh_update(1, skin.bounds(pal, mw, box) ? box : nullptr); scene.update_meshes(&u, 1, s); }\n'
            'int main() { static_assert(sizeof(hr_skin_desc) == 64, "hr_skin_desc"); hr_skin_desc d = hr_skin_desc();\n'
            '  std::vector<float> p, n; return hr::Skin::check(d) == HR_ERR_INVALID_ARG ? 0 : 1; }\n')
    with tempfile.NamedTemporaryFile("w", suffix=".cpp", delete=False) as f:
        f.write(code)
    try:
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), f.name])
    finally:
        os.unlink(f.name)


def refusal(sk, arrays, **fields):
    """(status, message) of hr_skin_check_desc over `arrays` with desc fields replaced"""
    a = sk.SkinArrays(arrays)
    d = a.desc()
    for k, v in fields.items():
        setattr(d, k, v)
    L = sk.lib()
    L.hr_last_error.restype = C.c_char_p
    st = L.hr_skin_check_desc(C.byref(d))
    return int(st), L.hr_last_error()


def test_check_desc_refuses_with_status_codes(sk):
    L = sk.lib()
    L.hr_last_error.restype = C.c_char_p
    good = sc.with_targets(sc.bar(3), 2, True)
    assert refusal(sk, good)[0] == 0
    assert L.hr_skin_check_desc(None) == INVALID_ARG and b"desc is NULL" in L.hr_last_error()
    for field in ("rest_positions", "rest_normals", "joints", "weights", "target_positions"):
        st, msg = refusal(sk, good, **{field: None})
        assert st == INVALID_ARG and field.encode() in msg and msg.startswith(b"hr_skin_check_desc"), (field, msg)
    assert refusal(sk, good, target_normals=None)[0] == 0          # normals need not morph
    assert refusal(sk, sc.bar(3), target_positions=None)[0] == 0   # no targets: no deltas
    for field, v, word in (("n_tris", 0, b"n_tris"), ("n_tris", -5, b"n_tris"), ("n_joints", 0, b"n_joints"), ("n_joints", -1, b"n_joints"),
                           ("n_joints", 65537, b"n_joints"), ("n_targets", -1, b"n_targets")):
        st, msg = refusal(sk, good, **{field: v})
        assert st == INVALID_ARG and word in msg, (field, v, msg)

    def edited(fn):
        a = sc.bar(3)
        a["joints"], a["weights"] = a["joints"].copy(), a["weights"].copy()
        fn(a)
        return a

    def set_w(i, k, v):
        return lambda a: a["weights"].reshape(-1, 4).__setitem__((i, k), F(v))

    def joint_out_of_range(a):
        a["joints"].reshape(-1, 4)[100, 0] = 3
        a["weights"].reshape(-1, 4)[100] = [1, 0, 0, 0]

    def all_zero(a):
        a["weights"].reshape(-1, 4)[191] = [0.0, -0.0, 0.0, 0.0]

    for fn, word in ((joint_out_of_range, b"joint index 3"), (set_w(7, 2, -0.25), b"negative"), (set_w(7, 3, np.nan), b"not finite"), (set_w(0, 0, np.inf), b"not finite"),
                     (set_w(0, 1, -np.inf), b"not finite"), (all_zero, b"all four weights are zero")):
        st, msg = refusal(sk, edited(fn))
        assert st == INVALID_ARG and word in msg, msg
    # a joint index past n_joints in a slot of weight zero is never read: accepted
    def skipped_slot(a):
        a["joints"][..., 3] = 65535
        a["weights"][..., 3] = F(-0.0)
    assert refusal(sk, edited(skipped_slot))[0] == 0
    # hr_skin_create and hr_skin_pose_host run the same checks first: refused before anything is allocated, with their own names
    bad = sk.SkinArrays(edited(all_zero))
    d, h = bad.desc(), C.c_void_p()
    L.hr_skin_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.hr_skin_create(None, C.byref(d), C.byref(h)) == INVALID_ARG and L.hr_last_error().startswith(b"hr_skin_create") and not h.value
    out = np.zeros((64, 3, 3), F)
    pal = sc.identity_palette(3)
    assert L.hr_skin_pose_host(C.byref(d), C.c_void_p(pal.ctypes.data), None, C.c_void_p(out.ctypes.data), None) == INVALID_ARG
    assert L.hr_last_error().startswith(b"hr_skin_pose_host")


def test_host_only_skin_info_bounds_refusals(sk):
    from hybrid_rendering_amd.api import HRError
    a = sc.with_targets(sc.bar(3), 2, False)
    s = sk.Skin(None, a)
    info = s.info()
    assert (info["n_tris"], info["n_joints"], info["n_targets"]) == (64, 3, 2) and info["lds_joint_cap"] >= 64
    w = a["weights"].astype(np.float64).sum(-1)
    assert info["max_weight_sum_error"] >= np.abs(w - 1.0).max() and info["max_weight_sum_error"] <= 2.0 ** -22
    pal = sc.bend_palette(3, 0.3)
    box = s.bounds(pal, [0.5, -0.5])
    assert box.shape == (2, 3) and (box[0] <= box[1]).all()
    for bad_pal, bad_mw in ((np.where(np.arange(48).reshape(3, 16) == 17, np.nan, pal), None), (pal, [np.inf, 0.0])):
        with pytest.raises(HRError, match="not finite"):
            s.bounds(bad_pal, bad_mw)
    L = sk.lib()
    L.hr_last_error.restype = C.c_char_p
    L.hr_skin_pose.argtypes = [C.c_void_p] * 4
    assert L.hr_skin_pose(s.h, C.c_void_p(pal.ctypes.data), None, None) == INVALID_ARG and b"host-only" in L.hr_last_error()
    s.close()
    # weights that sum to 0.9: no rounding-level box exists
    short = sc.bar(3)
    short["weights"] = (short["weights"].astype(np.float64) * 0.9).astype(F)
    s = sk.Skin(None, short)
    assert abs(s.info()["max_weight_sum_error"] - 0.1) < 1e-6
    L = sk.lib()
    L.hr_last_error.restype = C.c_char_p
    out = np.zeros(6, F)
    assert L.hr_skin_bounds(s.h, C.c_void_p(np.ascontiguousarray(pal).ctypes.data), None, C.c_void_p(out.ctypes.data)) == UNSUPPORTED
    assert b"bounds = NULL" in L.hr_last_error()
    s.close()
