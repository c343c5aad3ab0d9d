"""The numerical contract of include/hr_env_sources.h restated in numpy — numpy only: no GPU, no oracle, no library.

Contract 1 (equirect to cubemap): ``equirect_table`` is the host table's formula in float64; ``equirect_to_cube`` is the kernel in float32, every
operation written in the contract's order, so its result equals csrc/env_sources.hip's bit for bit when it is fed the library's own table.
Contract 2 (analytic sky): ``sky_coefficients`` is the host part in float64; ``sky_cube`` is the kernel's text in dtype F — in float64 it is the
reference the device's fp32 evaluation (with the device library's expf / acosf) is held to within a tolerance.  The texel directions, dot3 and
normalize3 are env_reference's (include/hr_env.h)."""
import numpy as np

import env_reference as er

FP16_MAX = 65504.0


def face_dirs64(S):
    """[6][S][S][3] float64: hr_env.h's face table over a = 2*((x + 0.5)/S) - 1, b likewise from y"""
    t = 2.0 * ((np.arange(S, dtype=np.float64) + 0.5) / S) - 1.0
    a, b = np.meshgrid(t, t)          # a along x (columns), b along y (rows)
    one = np.ones_like(a)
    return np.stack([np.stack([one, -b, -a], -1), np.stack([-one, -b, a], -1), np.stack([a, one, b], -1),
                     np.stack([a, -one, -b], -1), np.stack([a, -b, one], -1), np.stack([-a, -b, -one], -1)])


def equirect_table64(S):
    """[6][S][S][2] float64 (u, v) before the rounding to float32"""
    d = face_dirs64(S)
    u = np.arctan2(d[..., 2], d[..., 0]) / (2.0 * np.pi) + 0.5
    v = np.arccos(d[..., 1] / np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])) / np.pi
    return np.stack([u, v], -1)


def equirect_table(S):
    return equirect_table64(S).astype(np.float32)


def equirect_taps(table, w, h):
    """the kernel's addressing: (xa, xb, ya, yb, fx, fy, x0, y0) per cube texel, float32 arithmetic"""
    F = np.float32
    X = table[..., 0] * F(w) - F(0.5)
    Y = table[..., 1] * F(h) - F(0.5)
    xf, yf = np.floor(X), np.floor(Y)
    fx, fy = X - xf, Y - yf
    assert fx.dtype == F and fy.dtype == F
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    return x0 % w, (x0 + 1) % w, np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1), fx, fy, x0, y0


def stored(c):
    """c > 0 ? min(c, 65504) : 0 — a NaN becomes 0"""
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, np.where(c < c.dtype.type(FP16_MAX), c, c.dtype.type(FP16_MAX)), c.dtype.type(0))


def equirect_to_cube(table, img):
    """table [6][S][S][2] float32, img [h][w][>= 3] float32 -> the sky as fp16 bits, [6][S][S][4]"""
    F = np.float32
    img = np.asarray(img, F)
    h, w = img.shape[:2]
    xa, xb, ya, yb, fx, fy, _, _ = equirect_taps(table, w, h)
    gx, gy = F(1) - fx, F(1) - fy
    out = np.ones(table.shape[:3] + (4,), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            p = img[..., c]
            top = p[ya, xa] * gx + p[ya, xb] * fx
            bot = p[yb, xa] * gx + p[yb, xb] * fx
            out[..., c] = stored(top * gy + bot * fy)
    assert out.dtype == F
    return np.ascontiguousarray(out.astype(np.float16)).view(np.uint16)


# ---- contract 2 -------------------------------------------------------------------------------------------------------------------------
DEFAULT_SKY = dict(sun_dir=(0.3, 0.9, 0.2), turbidity=2.5, scale=0.1, ground_albedo=(0.2, 0.2, 0.2))
_MX = np.array([[0.00166, -0.00375, 0.00209, 0.0], [-0.02903, 0.06377, -0.03202, 0.00394], [0.11693, -0.21196, 0.06052, 0.25886]])
_MY = np.array([[0.00275, -0.00610, 0.00317, 0.0], [-0.04214, 0.08970, -0.04153, 0.00516], [0.15346, -0.26756, 0.06670, 0.26688]])


def perez_coefficients(T):
    """[3][5]: Y, x, y by A..E"""
    return np.array([[0.1787 * T - 1.4630, -0.3554 * T + 0.4275, -0.0227 * T + 5.3251, 0.1206 * T - 2.5771, -0.0670 * T + 0.3703],
                     [-0.0193 * T - 0.2592, -0.0665 * T + 0.0008, -0.0004 * T + 0.2125, -0.0641 * T - 0.8989, -0.0033 * T + 0.0452],
                     [-0.0167 * T - 0.2608, -0.0950 * T + 0.0092, -0.0079 * T + 0.2102, -0.0441 * T - 1.6537, -0.0109 * T + 0.0529]], np.float64)


def _perez64(c, theta, gamma):
    return (1.0 + c[0] * np.exp(c[1] / np.cos(theta))) * (1.0 + c[2] * np.exp(c[3] * gamma) + c[4] * np.cos(gamma) ** 2)


def sky_coefficients(sun_dir, turbidity, scale, ground_albedo):
    """the 24 values of the contract's `out` in float64 (the library rounds each to float32), and ground_albedo[2]"""
    s = np.asarray([np.float32(v) for v in sun_dir], np.float64)          # the parameters are floats in hr_sky_params
    s = s / np.sqrt((s * s).sum())
    T = float(np.float32(turbidity))
    ths = np.arccos(np.clip(s[1], 0.0, 1.0))
    co = perez_coefficients(T)
    chi = (4.0 / 9.0 - T / 120.0) * (np.pi - 2.0 * ths)
    tv, th = np.array([T * T, T, 1.0]), np.array([ths ** 3, ths ** 2, ths, 1.0])
    zen = [(4.0453 * T - 4.9710) * np.tan(chi) - 0.2155 * T + 2.4192, tv @ _MX @ th, tv @ _MY @ th]
    k = [zen[q] / _perez64(co[q], 0.0, ths) for q in range(3)]
    ga = [float(np.float32(v)) for v in ground_albedo]
    return np.concatenate([co.reshape(-1), k, s, [float(np.float32(scale)), ga[0], ga[1]]]).astype(np.float64), ga[2]


def sky_cube(S, coef, ground_b, F=np.float64):
    """the kernel's text in dtype F over the 24 coefficients: rgb [6][S][S][3] after the clamp, before the fp16 store"""
    co = np.asarray(coef).astype(F)
    N = er.normalize3(er.texel_dirs(S, F), F)
    ct = np.maximum(N[..., 1], F(0.02))
    cg = np.clip(er.dot3(N, co[18:21]), F(-1), F(1))
    g = np.arccos(cg)

    def perez(c, k):
        return (k * (F(1) + c[0] * np.exp(c[1] / ct))) * ((F(1) + c[2] * np.exp(c[3] * g)) + (c[4] * cg) * cg)

    Y, x, y = perez(co[0:5], co[15]), perez(co[5:10], co[16]), perez(co[10:15], co[17])
    X = (x / y) * Y
    Z = (((F(1) - x) - y) / y) * Y
    rgb = np.stack([(F(3.2404542) * X - F(1.5371385) * Y) - F(0.4985314) * Z, (F(-0.9692660) * X + F(1.8760108) * Y) + F(0.0415560) * Z,
                    (F(0.0556434) * X - F(0.2040259) * Y) + F(1.0572252) * Z], -1)
    rgb = rgb * co[21]
    ground = np.array([co[22], co[23], F(ground_b)], F)
    rgb = np.where((N[..., 1] < 0)[..., None], rgb * ground, rgb)
    assert rgb.dtype == F
    return stored(rgb)


def sky_reference(S, **params):
    """float64 all the way: [6][S][S][3]"""
    p = dict(DEFAULT_SKY, **params)
    coef, gb = sky_coefficients(p["sun_dir"], p["turbidity"], p["scale"], p["ground_albedo"])
    return sky_cube(S, coef, gb, np.float64)


def sun_at_elevation(deg, azimuth_deg=30.0):
    e, a = np.radians(deg), np.radians(azimuth_deg)
    return (float(np.cos(e) * np.cos(a)), float(np.sin(e)), float(np.cos(e) * np.sin(a)))


# the parameter sets of the coefficient test (CPU) and of the sky test (GPU): T x elevation, then a non-unit sun_dir, scale 0, a coloured ground
TURBIDITIES, ELEVATIONS = (1.7, 2.5, 6.0, 10.0), (90.0, 45.0, 5.0, -10.0)
GRID_SETS = [dict(sun_dir=sun_at_elevation(el), turbidity=T) for T in TURBIDITIES for el in ELEVATIONS]
EXTRA_SETS = [dict(sun_dir=(3.0, 9.0, 2.0)), dict(scale=0.0), dict(ground_albedo=(0.9, 0.1, 0.4), sun_dir=sun_at_elevation(20.0, 200.0))]
SKY_SETS = GRID_SETS + EXTRA_SETS


def equirect_images():
    """name -> float32 [h][w][4]: seeded noise in [0, 4) with one texel each of 1e6, +inf, NaN and -1 where the image has room for them"""
    out = {}
    for i, (w, h) in enumerate(((1, 1), (2, 1), (8, 4), (7, 5))):
        rng = np.random.RandomState(100 + i)
        img = np.ones((h, w, 4), np.float32)
        img[..., :3] = rng.uniform(0.0, 4.0, (h, w, 3)).astype(np.float32)
        if w * h >= 20:
            for k, val in enumerate((1e6, np.inf, np.nan, -1.0)):
                img[(k * 7 + 3) % h, (k * 5 + 1) % w, k % 3] = val
        out[f"{w}x{h}"] = img
    return out
