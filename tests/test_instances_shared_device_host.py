"""The device-side instance update without a GPU: the arithmetic both paths share (csrc/instance_math.h) in a stand-alone program under the address
and undefined-behaviour sanitizers (tests/instance_math_check.cpp — a binary of its own, nothing is loaded into Python), and the ABI of the three
entry points: declared, exported, mirrored with argtypes, refusing bad arguments as status codes before any device call."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid_rendering_amd", "csrc")
NEW = ("hr_scene_update_instances_device", "hr_scene_device_update_status", "hr_scene_device_update_stats")


def test_shared_arithmetic_under_sanitizers(tmp_path):
    """next_down / next_up / exponent_for against <cmath>; records and boxes of hostile matrices (zero, 1e-4 and 1e4 scales, a shear, condition
    1e6 / 9e6 / 1.1e7, overflow and underflow, an empty mesh) against the <cmath> restatement of the host code; the refit of a 601-instance top level
    depth by depth (the device kernels' order) against the host's slot order and against a <cmath> restatement of the node body (exponents,
    quantisation, clamps), byte for byte; no sanitizer report"""
    exe = str(tmp_path / "instance_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "instance_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("helpers:") and lines[1].startswith("records and boxes:") and "601 instances" in lines[2], r.stdout


def test_the_entry_points_are_declared_exported_and_mirrored():
    from hybrid_rendering_amd import api, build as hb
    hdr = open(os.path.join(ROOT, "include", "hr_api_stages.h")).read()
    assert "hr_scene_update_instances_device" not in open(os.path.join(ROOT, "include", "hr_api.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(hb.build())
    for s in NEW:
        assert re.search(r"hr_status\s+" + s + r"\s*\(", decl), s
        assert hasattr(L, s) and s in api.ABI_SYMBOLS and s in api.DEVICE_UPDATE_ARGTYPES, s
    assert "hr_scene_update_instances_device" in open(os.path.join(ROOT, "docs", "API_HISTORY.md")).read()
    assert [len(api.DEVICE_UPDATE_ARGTYPES[s]) for s in NEW] == [4, 4, 3]
    for name in ("update_device", "device_update_status", "device_update_stats"):
        assert callable(getattr(api.InstancedScene, name))
    pp = open(os.path.join(ROOT, "include", "hr", "passes.hpp")).read()
    assert "update_instances_device" in pp and "device_update_status" in pp and "device_update_stats" in pp
    assert "instances_shared_update.hip" in hb.OPTIONAL and os.path.exists(os.path.join(CSRC, "instances_shared_update.hip"))


def test_bad_arguments_are_status_codes_before_any_device_call():
    from hybrid_rendering_amd import api, build as hb
    L = C.CDLL(hb.build())
    L.hr_last_error.restype = C.c_char_p
    for s in NEW:
        getattr(L, s).argtypes = api.DEVICE_UPDATE_ARGTYPES[s]
    r, a, b, x, y = C.c_float(7.0), C.c_int32(7), C.c_int32(7), C.c_int64(7), C.c_int64(7)
    assert L.hr_scene_update_instances_device(None, None, None, None) == 1            # HR_ERR_INVALID_ARG
    assert b"hr_scene_update_instances_device" in L.hr_last_error()
    assert L.hr_scene_device_update_status(None, C.byref(r), C.byref(a), C.byref(b)) == 1
    assert L.hr_scene_device_update_stats(None, C.byref(x), C.byref(y)) == 1
    assert (r.value, a.value, b.value, x.value, y.value) == (7.0, 7, 7, 7, 7), "nothing is written on an error"
