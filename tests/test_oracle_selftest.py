"""The oracle's vectorised self-test mirror (orc_selftest_math / orc_selftest_compare) — what tests/test_gpu_device_math.py compares the device
with — pinned to the oracle's scalar entry points, to numpy, and to its own input generators.  CPU only."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32


@pytest.fixture(scope="module")
def po(oracle):
    return oracle


def _inputs(*cols):
    n = max(len(np.atleast_1d(c)) for c in cols)
    a = np.zeros((n, 8), F32)
    for k, c in enumerate(cols):
        a[:, k] = c
    return a


def _same(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _operands(seed, n=20_000):
    rng = np.random.RandomState(seed)
    bits = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F32)
    return np.concatenate([bits, rng.uniform(-100, 100, n).astype(F32), np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.4e-45, 88.0, -87.0, 4e9], F32)])


def test_mirror_matches_the_scalar_entry_points(po):
    L = po.lib()
    x = _operands(1)
    y = np.resize(np.array([0.0, 1.0, 2.2, 1 / 2.2, 32.0, 7.5, -1.0, np.inf], F32), len(x))
    inp = _inputs(x, y)
    sc = po.selftest_math(0, 0, len(x), inp, nout=2)
    s, c = C.c_float(), C.c_float()
    ex = po.selftest_math(0, 1, len(x), inp, nout=1)[0]
    lg = po.selftest_math(0, 2, len(x), inp, nout=1)[0]
    pw = po.selftest_math(0, 3, len(x), inp, nout=1)[0]
    h = po.selftest_math(0, 4, len(x), inp, nout=2)
    for i in range(0, len(x), 13):
        L.orc_sincos(C.c_float(float(x[i])), C.byref(s), C.byref(c))
        assert _same(sc[0, i], s.value) and _same(sc[1, i], c.value), x[i]
        assert _same(ex[i], L.orc_exp(float(x[i]))) and _same(lg[i], L.orc_log(float(x[i]))), x[i]
        assert _same(pw[i], L.orc_pow(float(x[i]), float(y[i]))), (x[i], y[i])
        assert h[0, i] == L.orc_f32_to_f16(float(x[i])) and _same(h[1, i], L.orc_f16_to_f32(L.orc_f32_to_f16(float(x[i])))), x[i]
    e = np.clip(x, -1.5, 1.5)
    od = po.selftest_math(0, 5, len(x), _inputs(e, e[::-1]), nout=3)
    out = (C.c_float * 3)()
    for i in range(0, len(x), 13):
        L.orc_oct_decode(C.c_float(float(e[i])), C.c_float(float(e[::-1][i])), out)
        assert all(_same(od[k, i], out[k]) for k in range(3)), (e[i], e[::-1][i])


def test_generators_match_explicit_inputs(po):
    first, n = 0x7f7fff00, 600                                     # runs through +max, +inf and into the NaNs
    gen = po.selftest_math(0, 0, n, gen=po.GEN_BITS, first=first, nout=2)
    x = np.arange(first, first + n, dtype=np.uint64).astype(np.uint32).view(F32)
    assert np.array_equal(gen.view(np.uint32), po.selftest_math(0, 0, n, _inputs(x), nout=2).view(np.uint32))
    first = 0x7bff7c00                                            # fp16 pairs: (ex, ey) = (bits & 0xffff, bits >> 16)
    gen = po.selftest_math(0, 5, n, gen=po.GEN_HALF2, first=first, nout=3)
    j = np.arange(first, first + n, dtype=np.uint64)
    ex = (j & 0xffff).astype(np.uint16).view(np.float16).astype(F32)
    ey = (j >> 16).astype(np.uint16).view(np.float16).astype(F32)
    assert _same(gen, po.selftest_math(0, 5, n, _inputs(ex, ey), nout=3)).all()
    # gen 3: denominators d_first, d_first + 1 ulp, ... each with every numerator; NaN entries draw random numerators in [1e-12, 3e5]
    num = np.array([0.0, 3e5, np.nan, np.nan], F32)
    p = po.selftest_params(z=1.0, d_first=0x3f800000, num=num)
    q = po.selftest_math(0, 8, 4000, gen=po.GEN_DIV, params=p, nout=1)[0]
    d = (0x3f800000 + np.arange(4000) // 4).astype(np.uint32).view(F32)
    n_ = q * d
    assert np.all(q[0::4] == 0.0) and np.allclose(n_[1::4], 3e5, rtol=1e-6)
    r = np.concatenate([n_[2::4], n_[3::4]])
    assert np.all((np.abs(r) >= 0.99e-12) & (np.abs(r) <= 3.01e5)) and (r < 0).mean() > 0.4 and (r > 0).mean() > 0.4
    assert np.log10(np.abs(r)).std() > 3.0                        # spread over the decades, not bunched


def test_compare_counts_mismatches_with_nan_equal_nan(po):
    first, n = 0x42b00000, 4096
    out = po.selftest_math(0, 1, n, gen=po.GEN_BITS, first=first, nout=1)
    assert po.selftest_compare(0, 1, po.GEN_BITS, first, n, out)[0] == 0
    nanout = po.selftest_math(0, 1, n, gen=po.GEN_BITS, first=0x7fc00000, nout=1)
    assert np.isnan(nanout).all()
    nanout[0, :10] = np.uint32(0xffc00001).view(F32)               # another NaN: equal
    assert po.selftest_compare(0, 1, po.GEN_BITS, 0x7fc00000, n, nanout)[0] == 0
    bad = out.copy()
    bad[0, [3, 77, 4000]] = np.nextafter(bad[0, [3, 77, 4000]], F32(np.inf))
    bad[0, 5] = -0.0 if out[0, 5] == 0.0 else np.nan
    cnt, idx = po.selftest_compare(0, 1, po.GEN_BITS, first, n, bad)
    assert cnt == 4 and list(idx) == [3, 5, 77, 4000]
    # fp16 planes (f2h bits as floats): any two fp16 NaN patterns are equal, nothing else is
    h = po.selftest_math(0, 4, 8, gen=po.GEN_BITS, first=0x7fc00000, nout=2)
    h[0, :] = 0x7e01
    assert po.selftest_compare(0, 4, po.GEN_BITS, 0x7fc00000, 8, h)[0] == 0
    h[0, 0] = 0x7c00
    assert po.selftest_compare(0, 4, po.GEN_BITS, 0x7fc00000, 8, h)[0] == 1


def test_mirror_f16_sqrt_div_against_numpy(po):
    """the oracle's fp32 -> fp16 rounding, sqrt and 1/x (modes 4 and 7) against numpy's float16 cast and float64, every 997th fp32 pattern"""
    x = np.arange(0, 1 << 32, 997, dtype=np.uint64).astype(np.uint32).view(F32)
    h = po.selftest_math(0, 4, len(x), _inputs(x), nout=1)[0].astype(np.uint32)
    with np.errstate(all="ignore"):
        ref = x.astype(np.float16).view(np.uint16)
        nan = (ref & 0x7c00 == 0x7c00) & (ref & 0x3ff != 0)
        assert ((h == ref) | (nan & (h & 0x7c00 == 0x7c00) & (h & 0x3ff != 0))).all()
        sr = po.selftest_math(0, 7, len(x), _inputs(x), nout=2)
        x64 = x.astype(np.float64)
        assert _same(sr[0], np.sqrt(x64).astype(F32)).all() and _same(sr[1], (1.0 / x64).astype(F32)).all()


def test_det_log_of_inf_and_nan(po):
    """regression: det_log(+inf) was 88.72, det_log(NaN) a finite value depending on the NaN's bits (89.13 for +qNaN, 266.6 for 0xffc00000)"""
    L = po.lib()
    assert L.orc_log(float("inf")) == float("inf")
    for b in (0x7fc00000, 0xffc00000, 0x7f800001):
        x = np.uint32(b).view(F32)
        assert np.isnan(po.selftest_math(0, 2, 1, _inputs([x]), nout=1)[0, 0]), hex(b)
    assert L.orc_log(3.4028234663852886e38) == pytest.approx(88.72283905206835, rel=1e-6)


def test_det_sincos_quadrant_beyond_int_range(po):
    """past |x| ~ 3.4e9 the quadrant is kf mod 4 in float arithmetic (0 there: kf is a multiple of 256); formerly (int)kf & 3, which the x86
    conversion (INT_MIN) happened to agree with and gfx950's saturating conversion (INT_MAX -> 3) did not"""
    x = np.array([3.5e9, 4e9, 1e10, 3.4028235e38, -3.5e9, -4e9], F32)
    sc = po.selftest_math(0, 0, len(x), _inputs(x), nout=2)
    kf = np.floor(x * F32(0.636619772367581) + F32(0.5))
    assert np.all(np.fmod(kf, 4) == 0)
    r = ((x - kf * F32(1.5703125)) - kf * F32(4.837512969970703125e-4)) - kf * F32(7.54978995489188e-8)
    with np.errstate(over="ignore", invalid="ignore"):
        z = r * r
        sp = ((F32(-1.9515295891e-4) * z + F32(8.3321608736e-3)) * z - F32(1.6666654611e-1)) * z * r + r
    assert _same(sc[0], sp).all()                                  # quadrant 0: sin = the sine polynomial, unswapped and unsigned
    inf = po.selftest_math(0, 0, 3, _inputs(np.array([np.inf, -np.inf, np.nan], F32)), nout=2)
    assert np.isnan(inf).all()


def test_fast_parity_modes_exist_and_approximations_do_not(po):
    """tu 1 (denoise_fast_resolve.hip): the parity helpers have a definition in the mirror; the hardware approximations (rcp, rsq, exp, log, pow,
    oct_unit) deliberately have none (their accuracy is measured against float64)"""
    inp = _inputs(np.ones(4, F32), np.ones(4, F32), np.ones(4, F32), np.ones(4, F32), np.ones(4, F32), np.ones(4, F32), np.ones(4, F32))
    p = po.selftest_params(m=np.eye(4), m2=np.eye(4), w=64, h=64)
    for which in (3, 5, 6, 7, 8, 9, 10, 11):
        po.selftest_math(1, which, 4, inp, params=p, nout=1)
    L = po.lib()
    for which in (0, 1, 2, 4):
        out = np.zeros(4, F32)
        assert L.orc_selftest_math(1, which, 0, 0, 4, inp.ctypes.data, p.ctypes.data, 1, out.ctypes.data) == -1
