"""include/hr_env.h without a GPU: the exported surface, argument validation, the host sample table, and the sanity of the numpy restatement of
the contract (tests/env_reference.py) that tests/test_gpu_env.py compares the device with bit for bit.  The framework passes hr_env replaces are
not in the reference tree, so the restatement has no external pin: the properties below (a constant sky stays constant, the LUT is a pair of
bounded monotone integrals, float32 and float64 agree) are what it is held to."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import env_reference as er
from hybrid_rendering_amd import synth_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


@pytest.fixture(scope="module")
def envlib():
    from hybrid_rendering_amd import build as hb, env
    hb.build()
    return env


def test_env_header_symbols_are_exported_and_mirrored(envlib):
    src = open(os.path.join(ROOT, "include", "hr_env.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hr_[a-z0-9_]+)\s*\(", src)))
    assert len(decl) == 11, decl
    L = envlib.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(envlib.ABI_SYMBOLS) == decl, set(envlib.ABI_SYMBOLS) ^ set(decl)
    # the mirror keeps to itself: the list tests/test_abi.py compares with the three older headers does not grow
    from hybrid_rendering_amd import api
    assert not set(envlib.ABI_SYMBOLS) & set(api.ABI_SYMBOLS)
    assert C.sizeof(envlib.hr_env_desc) == 20


def test_env_rejects_bad_arguments_with_status_codes(envlib):
    L = envlib.lib()
    L.hr_last_error.restype = C.c_char_p
    d = envlib.default_desc()
    assert (d.sky_size, d.prefiltered_size, d.prefiltered_levels, d.brdf_lut_size, d.n_samples) == (128, 128, 5, 128, 1024)
    h = C.c_void_p()

    def create(**kw):
        dd = envlib.default_desc()
        for k, v in kw.items():
            setattr(dd, k, v)
        st = L.hr_env_create(None, C.byref(dd), C.byref(h))
        return st, L.hr_last_error()

    # a good descriptor reaches the context check (there is no device here); a bad one is refused before it, by the field at fault
    st, msg = create()
    assert st == INVALID_ARG and msg.endswith(b"ctx"), msg
    for kw, word in ((dict(sky_size=96), b"sky_size"), (dict(sky_size=2), b"sky_size"), (dict(sky_size=4096, prefiltered_size=4096), b"sky_size"),
                     (dict(prefiltered_size=48), b"prefiltered_size"), (dict(sky_size=64, prefiltered_size=128), b"prefiltered_size"),
                     (dict(n_samples=100), b"n_samples"), (dict(n_samples=0), b"n_samples"), (dict(n_samples=8192), b"n_samples"),
                     (dict(prefiltered_size=8, prefiltered_levels=5), b"prefiltered_levels"), (dict(prefiltered_levels=0), b"prefiltered_levels"),
                     (dict(brdf_lut_size=0), b"brdf_lut_size"), (dict(brdf_lut_size=513), b"brdf_lut_size")):
        st, msg = create(**kw)
        assert st == INVALID_ARG and word in msg and not msg.endswith(b"ctx"), (kw, msg)
    assert create(prefiltered_size=8, prefiltered_levels=4)[1].endswith(b"ctx")      # log2(8) + 1 levels: allowed
    assert create(brdf_lut_size=5)[1].endswith(b"ctx")                               # the LUT need not be a power of two
    assert L.hr_env_create(None, None, C.byref(h)) == INVALID_ARG and L.hr_env_create(None, C.byref(d), None) == INVALID_ARG
    assert L.hr_env_update(None, None, None) == INVALID_ARG and L.hr_env_get(None, None) == INVALID_ARG
    assert L.hr_env_sh9_device(None, None) == INVALID_ARG and L.hr_env_read_sh9(None, None) == INVALID_ARG
    assert L.hr_env_set_profiling(None, 1) == INVALID_ARG and L.hr_env_get_stage_times(None, None) == INVALID_ARG
    assert L.hr_deferred_bind_sh9(None, None) == INVALID_ARG
    assert L.hr_env_destroy(None) == 0
    buf = (C.c_float * (4 * 128))()
    assert L.hr_env_sample_table(100, buf) == INVALID_ARG and L.hr_env_sample_table(64, None) == INVALID_ARG and L.hr_env_sample_table(0, buf) == INVALID_ARG


def test_environment_shim_compiles():
    """include/hr/environment.hpp is valid C++14 against hr_env.h and passes.hpp"""
    import subprocess
    import tempfile
    src = ('#include <hr/environment.hpp>\nint main() { hr_env_desc d = hr::Environment::default_desc(); float t[64 * 4];\n'
           '  return hr_env_sample_table(64, t) == HR_OK && d.n_samples > 0 && sizeof(hr::Environment) > 0 ? 0 : 1; }\n')
    with tempfile.NamedTemporaryFile("w", suffix=".cpp", delete=False) as f:
        f.write(src)
    try:
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), f.name])
    finally:
        os.unlink(f.name)


@pytest.mark.parametrize("n", [64, 192, 1024])
def test_sample_table_matches_the_contract(envlib, n):
    t = envlib.sample_table(n)
    i = np.arange(n)
    assert np.array_equal(t[:, 0].view(np.uint32), (i.astype(np.float32) / np.float32(n)).view(np.uint32))
    assert np.array_equal(t[:, 3].view(np.uint32), np.zeros(n, np.uint32))
    # the bit reversal, independently of env_reference: reverse the 32-character binary string
    rev = np.array([int(format(int(k), "032b")[::-1], 2) for k in i], np.uint64)
    assert np.array_equal(er.bitreverse32(i), rev.astype(np.uint32))
    phi = 2.0 * math.pi * (rev.astype(np.float64) * 2.0 ** -32)
    # the angle is exact: the library's (cos, sin) lies on the circle through numpy's to 1 fp32 ulp per component
    for col, want in ((1, np.cos(phi)), (2, np.sin(phi))):
        got, ref = t[:, col], want.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)).all(), (n, col)
    ref = er.sample_table(n)
    assert np.array_equal(ref[:, 0], t[:, 0]) and np.abs(ref - t).max() < 1e-6
    assert t[0].tolist() == [0.0, 1.0, 0.0, 0.0] and t[1, 1] == -1.0      # xi2(1) = 1/2: phi = pi


def _ulps16(a_bits, b_bits):
    """distance in fp16 steps between two arrays of non-negative finite fp16 bit patterns"""
    assert (a_bits < 0x7c00).all() and (b_bits < 0x7c00).all()
    return np.abs(a_bits.astype(np.int32) - b_bits.astype(np.int32))


@pytest.mark.parametrize("F", [np.float32, np.float64], ids=["f32", "f64"])
def test_reference_keeps_a_constant_sky_constant(F):
    S, levels, n = 8, 4, 64
    c = np.array([0.75, 0.3, 1.7], np.float16)      # 0.3 and 1.7 are not fp32-exact multiples of anything: the quotient has to round back
    sky = np.zeros((6, S, S, 4), np.float16)
    sky[..., :3], sky[..., 3] = c, 1.0
    sky = sky.view(np.uint16)
    table = er.sample_table(n)
    chain = er.prefiltered_chain(sky, S, levels, table, F)
    assert chain.shape == (er.chain_offsets(S, levels)[-1], 4)
    want = np.broadcast_to(np.append(c, np.float16(1.0)).view(np.uint16), chain.shape)
    assert _ulps16(chain, want).max() <= 1
    assert np.array_equal(chain[:, 3], want[:, 3])
    sh = er.sh9(sky, F)
    assert sh.dtype == F and (sh[:, 3] == 0).all()
    dc = c.astype(np.float64) * 0.282095 * 4.0 * math.pi
    assert np.allclose(sh[0, :3], dc, rtol=1e-5, atol=0)
    # the eight higher bands of a constant vanish: below 1e-2 of the constant term.  Measured at S = 8, max |band| / dc: 1.1e-16 in float64
    # (the cube's symmetry cancels them texel against texel, so the midpoint rule adds no error of its own), 5.9e-8 in float32; the constant
    # term's relative error is 6.6e-14 and 1.2e-7
    assert (np.abs(sh[1:, :3]) < 1e-2 * dc).all(), np.abs(sh[1:, :3] / dc).max()


def test_reference_level_zero_is_the_sky_and_the_chain_is_packed():
    sky = synth_env.sky_cubemap(size=8)
    table = er.sample_table(64)
    chain = er.prefiltered_chain(sky, 8, 4, table)
    off = er.chain_offsets(8, 4)
    assert off == [0, 384, 480, 504, 510] and len(chain) == 510
    assert np.array_equal(chain[:384], sky.reshape(-1, 4))
    # a smaller chain than the sky: level 0 is a fetch — every texel of it is one of the four sky texels its footprint covers
    sky16 = synth_env.sky_cubemap(size=16)
    c8 = er.prefiltered_chain(sky16, 8, 1, table).reshape(6, 8, 8, 4)
    quad = sky16.reshape(6, 8, 2, 8, 2, 4)
    assert ((c8[:, :, None, :, None, :] == quad).all(-1).any((2, 4))).all()
    # every texel is a weighted mean of sky texels with positive weights: nothing leaves the sky's range (one fp16 step for the rounded quotient),
    # and the roughest level is flatter than the sky
    val = chain.view(np.float16).astype(np.float32)
    rgb = sky.view(np.float16)[..., :3].astype(np.float32)
    assert val[:, :3].min() >= rgb.min() * (1 - 2.0 ** -10) and val[:, :3].max() <= rgb.max() * (1 + 2.0 ** -10)
    assert np.ptp(val[off[3]:, :3]) < np.ptp(rgb)


def test_reference_lut_is_a_bounded_monotone_split_sum():
    lut, n = 16, 1024
    table = er.sample_table(n)
    v32, v64 = er.brdf_lut_values(lut, table, np.float32), er.brdf_lut_values(lut, table, np.float64)
    assert v32.dtype == np.float32 and v64.dtype == np.float64
    b32, b64 = v32.astype(np.float16).view(np.uint16), v64.astype(np.float16).view(np.uint16)
    assert _ulps16(b32, b64).max() <= 1
    assert np.array_equal(er.brdf_lut(lut, table), b32)
    one_ulp = float(np.spacing(np.float16(1.0)))
    for v, stored in ((v32.astype(np.float16).astype(np.float64), True), (v32.astype(np.float64), False), (v64, False)):
        A, B = v[..., 0], v[..., 1]
        assert (A >= 0).all() and (B >= 0).all()
        assert (A + B <= 1.0 + one_ulp).all(), (A + B).max()
        # row 0 = the lowest roughness; columns = N.V.  Strictly increasing as computed; the fp16 store saturates at 1 toward N.V = 1
        assert (np.diff(A[0]) >= 0).all() if stored else (np.diff(A[0]) > 0).all(), A[0]
    # the corners the consumers know: smooth and head-on reflects everything at F0's scale, grazing moves the weight to the bias
    assert v64[0, -1, 0] > 0.9 and v64[0, -1, 1] < 0.01 and v64[0, 0, 1] > v64[0, -1, 1]
