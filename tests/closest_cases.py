"""Adversarial inputs for the two CLOSEST-HIT trace launches (k_ddgi_trace, k_refl_trace) and for k_ddgi_probe_update — the counterpart of
trace_cases.py, which does the same for the any-hit launches.  The builders are numpy only; the oracle's ray generation (`raygen`, bound at the
bottom) tells them the exact ray of every thread, and the geometry is then placed ON those rays: vertices, shared edges and fan hubs at
fl(o + t d) and 1 / 2 / 8 ulps beside it, planes at t_min = 0.001 and t_max = 10000 and ulps around them.  Every triangle has a material of its
own, so that the stored colour names the primitive that won.

    update_cases()                      the probe update (no tracing): dict(name, ddgi, rad, dd, prev_irr, prev_dep, first, shard, family [probe], aimed, dirs)
    ddgi_cases(raygen, child_boxes)     the DDGI trace: Case(name, ddgi, orientation, sd (SceneData), rays, family / ulps / own / tdist [probe][ray], knife, must_hit,
                                        first, infinite_bounces, shard)
    reflection_groups(raygen)           the reflections trace: [group]: dict(name, sd, frames); an RFrame carries its G-buffer, UBO, params and the same bookkeeping
                                        per thread of the padded 8x8 tile grid
    built_ddgi() / built_reflections()  the same, bound to the oracle's ray generation and the product's host BVH builder, built once per process
    expect_borders / update_reference   the probe update's expectations: the copy rule written down here, and the oracle over sentinel-filled atlases

All values are finite."""
import functools

import numpy as np

import ray_cases as rc
from hybrid_rendering_amd import synth, synth_env

F32 = np.float32
ULPS = (0, 1, -1, 2, -2, 8, -8)
EPS = F32(0.00000001)          # the probe update's weight threshold
SENTINEL = np.uint16(0x5a5a)   # what an untouched atlas texel must keep (fp16 203.25)


def half(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def f16(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(F32)


# ================================================================================================================ probe update
# The arithmetic of one (texel, ray) weight, restated in fp32 numpy to AIM the rays (orc_ddgi.cpp orc_ddgi_probe_update stays the reference:
# tests/test_closest_cases.py checks that this restatement agrees with it on the single-ray case).
def texel_dirs(side):
    """[side][side][3]: gi_oct_decode of the texel centres, [ly][lx]"""
    l = np.arange(side, dtype=F32)
    nc = ((l + F32(0.5)) * (F32(2.0) / F32(side)) - F32(1.0)).astype(F32)
    ox, oy = np.meshgrid(nc, nc)
    z = (F32(1.0) - np.abs(ox) - np.abs(oy)).astype(F32)
    snz = lambda k: np.where(k >= 0, F32(1), F32(-1)).astype(F32)
    nx, ny = ((F32(1) - np.abs(oy)) * snz(ox)).astype(F32), ((F32(1) - np.abs(ox)) * snz(oy)).astype(F32)
    x, y = np.where(z < 0, nx, ox).astype(F32), np.where(z < 0, ny, oy).astype(F32)
    inv = (F32(1) / np.sqrt(((x * x + y * y).astype(F32) + z * z).astype(F32))).astype(F32)
    return np.stack([x * inv, y * inv, z * inv], -1).astype(F32)


def dot32(t, d):
    return (((t[..., 0] * d[..., 0]).astype(F32) + (t[..., 1] * d[..., 1]).astype(F32)).astype(F32) + (t[..., 2] * d[..., 2]).astype(F32)).astype(F32)


def powi32(x, n):
    """det_powi (orc_math.h): square and multiply, every product rounded"""
    r, b = np.ones_like(x, F32), np.asarray(x, F32).copy()
    while n > 0:
        if n & 1:
            r = (r * b).astype(F32)
        b = (b * b).astype(F32)
        n >>= 1
    return r


def weight32(t, d, sharpness=None):
    """the weight of ray direction d for texel direction t: max(0, dot) for the irradiance atlas, that to an INTEGER sharpness for the depth atlas"""
    dp = np.maximum(F32(0.0), dot32(t, d))
    return dp if sharpness is None else powi32(dp, int(sharpness))


@functools.lru_cache(maxsize=None)
def _irr_knife(side):
    """per irradiance texel two fp16 SUBNORMAL directions (components j * 2^-24, |j| <= 8): the one whose dp is the smallest >= 1e-8 and the one
    whose dp is the largest < 1e-8 — found by search over the 17^3 lattice.  -> [side*side][2][3] float32"""
    r = np.arange(-8, 9)
    g = (np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3).astype(F32) * F32(2.0 ** -24)).astype(F32)
    out = np.zeros((side * side, 2, 3), F32)
    for k, t in enumerate(texel_dirs(side).reshape(-1, 3)):
        dp = weight32(t[None], g)
        above, below = np.where(dp >= EPS, dp, np.inf), np.where(dp < EPS, dp, -np.inf)      # side 2: no dp in (0, 1e-8), the largest below is 0
        out[k, 0], out[k, 1] = g[np.argmin(above)], g[np.argmax(below)]
        assert np.isfinite(above.min()) and np.isfinite(below.max())
    return out


@functools.lru_cache(maxsize=None)
def _depth_knife(side, sharpness):
    """per depth texel two SHORT fp16 directions s * texel_dir (|d| ~ 0.69 for sharpness 50, ~ 0.61 for 37), s searched over a ladder of 2e-4
    steps: the one whose dp^sharpness is the smallest >= 1e-8 and the one whose is the largest < 1e-8.  -> [side*side][2][3] float32"""
    s0 = 1e-8 ** (1.0 / sharpness)
    ladder = s0 * (1.0 + 2e-4 * np.arange(-24, 25))
    out = np.zeros((side * side, 2, 3), F32)
    for k, t in enumerate(texel_dirs(side).reshape(-1, 3)):
        d = f16(half(t[None].astype(np.float64) * ladder[:, None]))
        w = weight32(t[None], d, sharpness)
        above, below = np.where(w >= EPS, w, np.inf), np.where(w < EPS, w, -np.inf)
        out[k, 0], out[k, 1] = d[np.argmin(above)], d[np.argmax(below)]
        assert np.isfinite(above.min()) and np.isfinite(below.max())
    return out


UPDATE_FAMILIES = ("irr_knife", "depth_knife", "one_ray", "all_skipped", "distances", "bulk", "exact_tie")
# EXACT ties: fp16 directions (bit patterns) whose fp32 dot product with a texel direction of side 12 is exactly 1e-8f.  The texels are
# four whose z is the rounding residue of 1 - |x| - |y| (-6.5e-8, -1.3e-7): two large products cancel and the third, tiny against that z,
# places the last bits.  search_exact_ties(12) below reproduces them (tests/test_closest_cases.py runs it, and runs it over sides 2, 7, 8 and 16,
# where it finds none).
TIE_SIDE = 12
TIES = ((71, (0x805b, 0x83eb, 0x223a)), (71, (0x805a, 0x83e0, 0x223a)), (83, (0x8067, 0x046f, 0x1e3a)), (83, (0x8064, 0x044e, 0x1e3a)),
        (137, (0x83eb, 0x805b, 0x223a)), (137, (0x83e0, 0x805a, 0x223a)), (138, (0x040c, 0x805e, 0x1e3a)), (138, (0x0417, 0x805f, 0x1e3a)))
def search_exact_ties(side, texels=None):
    """[(texel, (x, y, z) fp16 bits)]: directions whose weight on a texel of `side` is exactly 1e-8f, found as follows.  The weight is
    fl(fl(tx dx + ty dy) + tz dz).  For every fp16 dx with |tx dx| < 0.25 (beyond that an ulp of the product exceeds the threshold) take the
    four fp16 dy nearest to -tx dx / ty, so that the first sum q all but cancels, then the two fp16 dz nearest to (1e-8 - q) / tz, and keep the
    triples whose weight IS 1e-8f.  A search, not a proof: it covers the directions that reach the threshold by this cancellation."""
    h16 = np.arange(1, 0x7c00, dtype=np.uint16).view(np.float16).astype(F32)
    hs = np.sort(np.concatenate([-h16, [F32(0)], h16]).astype(F32))
    near = lambda v: np.clip(np.searchsorted(hs, v), 1, len(hs) - 1)
    out = []
    td = texel_dirs(side).reshape(-1, 3)
    for k in (range(len(td)) if texels is None else texels):
        t = td[k]
        if (t == 0).any():
            continue
        dx = hs[(np.abs(hs.astype(np.float64) * float(t[0])) < 0.25) & (hs != 0)]
        px = (t[0] * dx).astype(F32)
        iy = near((-px.astype(np.float64) / float(t[1])).astype(F32))
        for oy in (-2, -1, 0, 1):
            dy = hs[np.clip(iy + oy, 0, len(hs) - 1)]
            q = (px + (t[1] * dy).astype(F32)).astype(F32)
            iz = near(((EPS.astype(np.float64) - q.astype(np.float64)) / float(t[2])).astype(F32))
            for oz in (-1, 0):
                dz = hs[np.clip(iz + oz, 0, len(hs) - 1)]
                d = np.stack([dx, dy, dz], -1)
                for i in np.flatnonzero(weight32(t[None], d) == EPS):
                    out.append((int(k), tuple(int(b) for b in half(d[i]))))
    return sorted(set(out))


#                name        counts   R   depth irr sharp hysteresis first  shard (z0, z1)
UPDATE_CONFIGS = (("r1",     (3, 2, 2), 1,   2,  2, 50.0, 0.98, True,  None),
                  ("r3",     (2, 3, 2), 3,   8,  7, 37.0, 0.0,  False, None),
                  ("r255",   (3, 2, 2), 255, 9,  8, 50.0, 1.0,  False, None),
                  ("r256",   (2, 3, 2), 256, 11, 16, 37.0, 0.98, False, None),
                  ("r257",   (3, 2, 2), 257, 12, 2, 50.0, 0.98, True,  (1, 2)),
                  ("r513",   (2, 3, 2), 513, 16, 8, 50.0, 0.98, False, (1, 2)),
                  # beyond the listed sizes: weights EXACTLY on the threshold (irradiance side 12; depth side 12 with sharpness 1, where the weight
                  # is the dot product itself) — alone in their probe (the total weight is exactly 1e-8: not normalised) and beside an ordinary ray
                  ("tie_r1", (3, 2, 2), 1,   12, 12, 1.0,  0.98, True,  None),
                  ("tie_r2", (2, 3, 2), 2,   12, 12, 1.0,  0.0,  False, None))


def distance_values(max_distance):
    """0, -0, negative, the trace's miss value, and max_distance + 0.01 (where min(max_distance, d - 0.01) changes sides) +- fp16 ulps"""
    m = np.float16(float(max_distance) + 0.01)
    lad = [m]
    for _ in range(3):
        lad = [np.nextafter(lad[0], np.float16(-np.inf))] + lad + [np.nextafter(lad[-1], np.float16(np.inf))]
    return np.array([0.0, -0.0, -1.0, -0.99, -3.5, 10000.0, 0.01, 0.0100021, 0.5] + [float(v) for v in lad], np.float16)


def update_case(name, counts, R, ds, isz, sharp, hyst, first, shard, seed):
    rng = np.random.RandomState(seed)
    ddgi = synth_env.ddgi_uniforms((0.0, 0.0, 0.0), (4.0, 4.0, 4.0), probe_counts=counts, rays_per_probe=R, hysteresis=hyst, depth_sharpness=sharp,
                                   irradiance_oct_size=isz, depth_oct_size=ds)
    n = int(np.prod(counts))
    tie = name.startswith("tie")
    fam = np.array([UPDATE_FAMILIES.index("exact_tie") if tie else i % (len(UPDATE_FAMILIES) - 1) for i in range(n)], np.int16)
    d = np.zeros((n, R, 3), F32)
    dist = rng.uniform(0.05, 1.4 * float(ddgi["max_distance"]), (n, R)).astype(np.float16)
    rad = rng.uniform(0.0, 4.0, (n, R, 4)).astype(np.float16)
    rad[..., 3] = 0
    # aimed[probe][ray] = (atlas 0 irradiance / 1 depth, texel, side 0 taken / 1 skipped), -1 where the ray is not aimed
    aimed = np.full((n, R, 3), -1, np.int32)
    ik, dk = (None, None) if tie else (_irr_knife(isz), _depth_knife(ds, sharp))
    dvals = distance_values(ddgi["max_distance"])
    for p in range(n):
        f = UPDATE_FAMILIES[fam[p]]
        if f == "irr_knife":
            for r in range(R):
                k, s = (r + p) % (isz * isz), ((r + p) // (isz * isz) + r) % 2
                d[p, r], aimed[p, r] = ik[k, s], (0, k, s)
        elif f == "depth_knife":
            for r in range(R):
                k, s = (r + 5 * p) % (ds * ds), ((r + 5 * p) // (ds * ds) + r) % 2
                d[p, r], aimed[p, r] = dk[k, s], (1, k, s)
        elif f == "one_ray":
            # ONE ray with a direction, at a position that is the last of a batch / of the unroll tail where R allows; the other rays' direction is 0
            nth = p // (len(UPDATE_FAMILIES) - 1)      # the probe's ordinal among the one_ray probes
            r = ((255, R - 1) if R > 256 else (R - 1, min(2, R - 1)))[nth % 2]      # the last slot of the first LDS batch, of the unroll tail; slot 2
            k = p % (isz * isz)
            s = (p // (len(UPDATE_FAMILIES) - 1)) % 2     # the probe's total weight: just over 1e-8 on the aimed texel, or nothing taken there
            d[p, r], aimed[p, r] = ik[k, s], (0, k, s)
        elif f == "exact_tie":
            k, bits = TIES[p % len(TIES)]
            d[p, 0], aimed[p, 0] = f16(np.array(bits, np.uint16)), (0, k, 0)
            rad[p, 0, 0:3] = (60000.0, 30000.0, 1000.0)      # 0.95 * 60000 * 1e-8 is an fp16 value far from 0: taken-and-not-normalised shows
            dist[p, 0] = np.float16(5.0 + 0.125 * p)
            if R > 1:
                t = texel_dirs(TIE_SIDE).reshape(-1, 3)[k]
                d[p, 1], rad[p, 1, 0:3] = f16(half(t * F32(0.5))), (0.01, 0.02, 0.03)
        elif f == "all_skipped":
            d[p] = 0.0
            d[p, ::2, 2] = F32(-0.0)
        else:
            v = rng.normal(size=(R, 3))
            d[p] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
            if f == "distances":
                dist[p] = dvals[(np.arange(R) + p) % len(dvals)]
    dd = np.zeros((n, R, 4), np.uint16)
    dd[..., 0:3] = half(d)
    knife = aimed[..., 0] >= 0
    assert np.array_equal(f16(dd[..., 0:3])[knife], d[knife]), "an aimed direction is not an fp16 value"
    d = f16(dd[..., 0:3])
    dd[..., 3] = dist.view(np.uint16)
    iw, ih, dw, dh = (int(ddgi[k]) for k in ("irradiance_texture_width", "irradiance_texture_height", "depth_texture_width", "depth_texture_height"))
    prev_irr = rng.uniform(0.0, 3.0, (ih, iw, 4)).astype(np.float16).view(np.uint16)
    prev_dep = rng.uniform(0.0, 3.0, (dh, dw, 2)).astype(np.float16).view(np.uint16)
    return dict(name=name, ddgi=ddgi, R=R, rad=np.ascontiguousarray(rad.view(np.uint16)), dd=dd, prev_irr=prev_irr, prev_dep=prev_dep, first=first, shard=shard,
                family=fam, aimed=aimed, dirs=d)


@functools.lru_cache(maxsize=1)
def update_cases():
    return [update_case(*c, seed=100 + i) for i, c in enumerate(UPDATE_CONFIGS)]


def cell_rows(side, z0, z1):
    """the atlas rows of the probe slabs z0 .. z1 - 1 (borders included)"""
    return slice(1 + z0 * (side + 2), 1 + z1 * (side + 2))


def expect_borders(atlas, side, counts):
    """The atlas with every probe's border rewritten FROM ITS INTERIOR by the copy rule, written down here and not taken from any implementation:
    a border texel of an edge shows the interior texel beside the edge, mirrored about the edge's middle; a corner texel shows the interior
    corner diagonally opposite.  In cell coordinates 0 .. S + 1 (interior 1 .. S):
        (i, 0) <- (S + 1 - i, 1)      (i, S + 1) <- (S + 1 - i, S)      (0, j) <- (1, S + 1 - j)      (S + 1, j) <- (S, S + 1 - j)      i, j in 1 .. S
        (0, 0) <- (S, S)      (S + 1, 0) <- (1, S)      (0, S + 1) <- (S, 1)      (S + 1, S + 1) <- (1, 1)"""
    out, S = atlas.copy(), side
    i = np.arange(1, S + 1)
    for gy in range(counts[2]):
        for gx in range(counts[0] * counts[1]):
            c = out[1 + gy * (S + 2): 1 + (gy + 1) * (S + 2), 1 + gx * (S + 2): 1 + (gx + 1) * (S + 2)]      # [y][x], a view
            c[0, i], c[S + 1, i] = c[1, S + 1 - i], c[S, S + 1 - i]
            c[i, 0], c[i, S + 1] = c[S + 1 - i, 1], c[S + 1 - i, S]
            c[0, 0], c[0, S + 1], c[S + 1, 0], c[S + 1, S + 1] = c[S, S], c[S, 1], c[1, S], c[1, 1]
    return out


def update_reference(case):
    """(irradiance atlas, depth atlas) of the oracle (orc_ddgi_probe_update + orc_ddgi_border_update) over sentinel-filled atlases: the texels no
    stage writes (the outer one-texel frame; with a shard, the slabs outside it) keep the sentinel"""
    from oracle import pyoracle_ddgi as od
    out = []
    for depth_probe, prev in ((False, case["prev_irr"]), (True, case["prev_dep"])):
        full = od.border_update(case["ddgi"], depth_probe, _probe_update_into(case, depth_probe, prev))
        if case["shard"] is not None:
            side = int(case["ddgi"]["depth_probe_side_length" if depth_probe else "irradiance_probe_side_length"])
            rows = cell_rows(side, *case["shard"])
            kept = np.full_like(full, SENTINEL)
            kept[rows] = full[rows]
            full = kept
        out.append(full)
    return out


def _probe_update_into(case, depth_probe, prev):
    import ctypes as C
    from oracle.pyoracle import _p, c_u16p, lib
    from oracle.pyoracle_ddgi import _ddgi_ptr
    out = np.full_like(prev, SENTINEL)
    lib().orc_ddgi_probe_update(_ddgi_ptr(case["ddgi"]), C.c_int(int(depth_probe)), C.c_int(int(case["first"])), _p(case["rad"], c_u16p), _p(case["dd"], c_u16p),
                                _p(prev, c_u16p), _p(out, c_u16p))
    return out


def interior(atlas, side, counts, probe):
    """the [side][side] interior texels of one probe (a view)"""
    gx, gy = probe % (counts[0] * counts[1]), probe // (counts[0] * counts[1])
    return atlas[2 + gy * (side + 2): 2 + gy * (side + 2) + side, 2 + gx * (side + 2): 2 + gx * (side + 2) + side]


# ================================================================================================================ scenes with one material per triangle
def light(direction=(0.3, 0.5, 0.8), intensity=1.0, radius=0.0):
    """a directional light with a unit direction TO the light; intensity 1 keeps every lit colour under the reflections' 0.7 clamp"""
    d = np.asarray(direction, np.float64)
    L = np.zeros(16, F32)
    L[0:3], L[3], L[7], L[8:11] = (d / np.linalg.norm(d)).astype(F32), intensity, radius, 1.0
    return L


def plain_ubo(lgt, cam=(0.0, 0.0, 0.0)):
    u = np.zeros((), synth.UBO_DTYPE)
    for k in ("view_inverse", "proj_inverse", "view_proj_inverse", "prev_view_proj", "view_proj"):
        u[k] = np.eye(4, dtype=F32).reshape(16)
    u["cam_pos"][0:3] = cam
    u["light"] = lgt
    return u


def materials_for(n, metallic=None):
    """[n][8]: albedo rgb, metallic, roughness, emissive rgb — every triangle its own albedo (three incommensurable steps, spaced far beyond an
    fp16 ulp of the lit colour), roughness and, cycling, metallic 0 / 0.5 / 1"""
    i = np.arange(1, n + 1, dtype=np.float64)
    m = np.zeros((n, 8), F32)
    m[:, 0], m[:, 1], m[:, 2] = 0.15 + 0.6 * ((i * 0.6180339887) % 1.0), 0.15 + 0.6 * ((i * 0.7548776662) % 1.0), 0.15 + 0.6 * ((i * 0.5698402910) % 1.0)
    m[:, 3] = np.asarray((0.0, 0.5, 1.0))[np.arange(n) % 3] if metallic is None else metallic
    m[:, 4] = 0.2 + 0.7 * ((i * 0.3819660113) % 1.0)
    return m


def scene_of(tris, name, metallic=None, facing=None):
    """SceneData over `tris` with geometric vertex normals ((0,0,1) for a triangle without area), turned to the side `facing` [n][3] names where it
    is not zero, and material i for triangle i"""
    tris = np.ascontiguousarray(tris, F32)
    v = tris.astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(l > 0, n / np.where(l > 0, l, 1.0), (0.0, 0.0, 1.0))
    if facing is not None:
        n = np.where(((n * facing).sum(1) < 0)[:, None], -n, n)
    normals = np.ascontiguousarray(np.repeat(n[:, None, :], 3, 1), F32)
    return synth.SceneData(tris, normals, np.arange(len(tris), dtype=np.uint32), np.ones(len(tris), np.uint32), materials_for(len(tris), metallic), name)


def coded_sky(size=4):
    """[6][S][S][4] fp16: a texel holds where it is — (face, iy, ix) folded into three small distinct values under 0.7"""
    t = np.zeros((6, size, size, 4), np.float64)
    f, iy, ix = np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing="ij")
    t[..., 0], t[..., 1], t[..., 2], t[..., 3] = 0.05 + 0.1 * f, 0.05 + 0.15 * iy / size, 0.05 + 0.15 * ix / size, 1.0
    return np.ascontiguousarray(half(t))


def coded_atlases(ddgi):
    """previous irradiance / depth atlases whose texels carry their position: (irradiance [h][w][4], depth [h][w][2]) fp16 bits"""
    iw, ih, dw, dh = (int(ddgi[k]) for k in ("irradiance_texture_width", "irradiance_texture_height", "depth_texture_width", "depth_texture_height"))
    y, x = np.mgrid[0:ih, 0:iw]
    irr = np.stack([0.05 + 0.01 * (x % 16), 0.05 + 0.01 * (y % 16), 0.1 + 0.005 * ((x + y) % 8), np.ones_like(x, np.float64)], -1)
    y, x = np.mgrid[0:dh, 0:dw]
    mean = 2.0 + 0.25 * ((x + 2 * y) % 16)
    dep = np.stack([mean, mean * mean + 0.25 + 0.05 * (x % 4)], -1)
    return np.ascontiguousarray(half(irr)), np.ascontiguousarray(half(dep))


# ================================================================================================================ DDGI trace
import trace_cases as tc      # on_ray_construct, cover, background, prune_near_rays: the constructs around an axis ray

AXIS_KINDS = tc.EDGE_KINDS + ("pair",)      # pair: two coplanar triangles over the ray — equal t, the lower index wins
DIAG_Z = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1], F32)      # column-major diag(0, 0, 1): every direction is (0, 0, +-1)


def _grid(counts, R, lo=(0.0, 0.0, 0.0), ext=8.0, **more):
    c = np.asarray(counts)
    hi = np.asarray(lo, np.float64) + ext * np.maximum(c - 2, 1)
    return synth_env.ddgi_uniforms(lo, hi, probe_counts=counts, rays_per_probe=R, normal_bias=0.1, **more)


class Case(dict):
    def of(self, name):
        return self["family"] == self["names"].index(name)

    def label(self, p, r):
        return self["names"][int(self["family"][p, r])]


def _new_case(name, ddgi, orientation, raygen, **more):
    rays = raygen(ddgi, orientation)
    n, R = rays.shape[:2]
    return Case(name=name, ddgi=ddgi, orientation=np.ascontiguousarray(orientation, F32), rays=rays, family=np.zeros((n, R), np.int16), names=["plain"],
                ulps=np.zeros((n, R), np.int16), own=np.full((n, R, 2), -1, np.int32), tdist=np.zeros((n, R), F32), knife={}, must_hit=(), light=light(), first=True, infinite_bounces=0,
                shard=None, **more)


def _mark(c, sel, name, ulps=0, own=None):
    if name not in c["names"]:
        c["names"].append(name)
    c["family"][sel] = c["names"].index(name)
    c["ulps"][sel] = ulps
    if own is not None:
        c["own"][sel] = own


def length_tie(j, off):
    """t such that fl(0.001f + t) is exactly the midpoint of the fp16 values 1 + j 2^-10 and 1 + (j + 1) 2^-10 (off = 0: the stored distance
    rounds to the even one), or `off` fp32 ulps beside that midpoint"""
    want = rc.step_ulps(F32(1.0 + j * 2.0 ** -10 + 2.0 ** -11), off)[()]
    t0 = F32(want - F32(0.001))
    for e in (0, 1, -1, 2, -2, 3, -3):
        t = rc.step_ulps(t0, e)[()]
        if F32(F32(0.001) + t) == want:
            return t
    raise AssertionError("no t puts 0.001f + t on the tie")


def ddgi_axis_case(raygen, name, counts, R, variant):
    """orientation diag(0,0,1), even R, the grid's bottom slab at z == 0 exactly: every ray of a probe runs along +z or -z through the probe, so
    vertices, shared edges, fan hubs and coplanar pairs lie EXACTLY on rays, and a plane z = +-t is hit at exactly t from the bottom slab.
      bottom slab, up:    a cover at z = t_min stepped by ulps (closer than everything else; a miss goes on to what lies above)
      bottom slab, down:  a cover at z = -t_max stepped by ulps
      top slab, up / down: one on-ray construct (vertex, edge, backface, shared edge, hub, zero area, pair), its feature stepped by ulps
    One top-slab probe also lies IN the plane of a triangle that holds both of its rays (coplanar rays: never a hit)."""
    ddgi = _grid(counts, R)
    c = _new_case(name, ddgi, DIAG_Z, raygen, tie_tris=[])
    rays = c["rays"]
    d = rays[..., 4:7]
    # x and y are exactly 0: the rays run exactly along z.  |d.z| is f.z * (1 / sqrt(f.z * f.z)): 1 or an ulp beside it
    assert (d[..., 0:2] == 0).all() and (np.abs(np.abs(d[..., 2]) - 1) <= 2.0 ** -23).all() and (np.abs(d[..., 2]) == 1).mean() > 0.5, "diag(0,0,1) does not give (0,0,+-1)"
    slab = counts[0] * counts[1]
    tris, n_tris, facing = [], 0, []      # facing: per triangle the side its normal turns to — where its ray comes from (a hit from behind is unlit: 0)
    for p in range(rays.shape[0]):
        o = rays[p, 0, 0:3]
        for sgn in (1, -1):
            rsel = np.zeros(rays.shape[:2], bool)
            rsel[p] = np.sign(d[p, :, 2]) == sgn
            i = 2 * p + (sgn < 0) + 5 * variant
            k = ULPS[i % len(ULPS)]
            if p < slab:
                assert o[2] == 0
                if sgn > 0:
                    # behind the t_min cover a second one at a height whose stored distance, fp16(0.001f + t), is a rounding TIE (or an fp32
                    # ulp beside one): the rays that pass the first cover (t <= t_min) hit it at exactly that t where d.z == 1
                    tie = tc.cover(o, length_tie(i % 6, (0, 0, 1, -1)[(i // 6) % 4]), s=0.375, flip=bool(i % 2))
                    c["tie_tris"].append(n_tris + 1)
                    t, fam = np.concatenate([tc.cover(o, rc.step_ulps(F32(0.001), k)[()], s=0.5, flip=bool(i % 2)), tie]), "tmin"
                else:
                    t, fam = tc.cover(o, F32(-rc.step_ulps(F32(10000.0), k)[()]), s=0.5, flip=bool(i % 2)), "tmax"
            else:
                # slot j of the 12 * (number of axis cases) top-slab rays: the kinds cycle fastest, every kind meets every ulp step and both sides
                j = 2 * (p - slab) + (sgn < 0) + 2 * slab * variant
                fam, m = AXIS_KINDS[j % len(AXIS_KINDS)], j // len(AXIS_KINDS)
                k = ULPS[m % len(ULPS)]
                z = F32(o[2] + sgn * (2.0 + 0.5 * (i % 3)))
                t = np.concatenate([tc.cover(o, z, s=0.25), tc.cover(o, z, s=0.375, flip=True)]) if fam == "pair" else tc.on_ray_construct(fam, o, z, k, m)
            _mark(c, rsel, fam, k, (n_tris, 1 if fam == "tmin" else len(t)))      # t_min: the first cover is the family's own, the tie cover lies behind it
            tris.append(t)
            facing.append(np.tile((0.0, 0.0, -float(sgn)), (len(t), 1)))
            n_tris += len(t)
    # the last probe lies in the plane x == o.x of a triangle that holds its up and its down ray
    o = rays[-1, 0, 0:3]
    tris.append(np.array([[(o[0], o[1] - 0.125, o[2] - 1.0), (o[0], o[1] + 0.125, o[2] - 1.0), (o[0], o[1], o[2] + 1.5)]], F32))
    facing.append(np.zeros((1, 3)))
    c["coplanar_tri"] = n_tris
    c["knife"] = {k: "hit" for k in ("tmin", "tmax", "vertex", "edge", "backface")}
    c["must_hit"] = ("shared_edge", "hub", "pair")
    c["sd"] = scene_of(np.concatenate(tris), name, facing=np.concatenate(facing))
    return c


def rotation(seed, scale=1.0):
    return np.ascontiguousarray(synth_env.random_orientation(np.random.RandomState(seed)) * F32(scale), F32)


ROT_KINDS = ("rot_vertex", "rot_shared_edge", "rot_hub", "rot_pair", "rot_vertex", "rot_far")


def _frame_of(d):
    d = np.asarray(d, np.float64)
    e1 = np.cross(d, (1.0, 0.0, 0.0) if abs(d[0]) < 0.9 else (0.0, 1.0, 0.0))
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(d, e1)


def rot_construct(kind, o, d, t, k, i, size=0.2):
    """triangles across the ray o + t d around q = fl(o + t d):
      rot_vertex        ONE triangle with a vertex at q stepped by k ulps along the axis in which d is smallest: to one side of it the ray misses
      rot_shared_edge   two triangles sharing an edge through q (closed around the ray: a hit for every small k)
      rot_hub           a closed fan of 5 .. 7 triangles around q
      rot_pair          the SAME triangle twice (equal t, u, v: the lower index wins)
      rot_far           one triangle across the ray at t ~ 9000 (most of the way to t_max)"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    q = (o + t * d).astype(F32)
    e1, e2 = _frame_of(d)
    a = int(np.argmin(np.abs(d)))
    qk = q.copy()
    qk[a] = rc.step_ulps(q[a], k)
    if kind == "rot_vertex":
        # the triangle opens from its vertex along axis a as seen across the ray: k > 0 moves the vertex past the ray (a miss), k < 0 puts the ray inside
        e1 = -np.asarray(d) * d[a]
        e1[a] += 1.0
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(d, e1)
    P = lambda u, v: (q.astype(np.float64) + size * (u * e1 + v * e2)).astype(F32)
    if kind == "rot_vertex":
        return np.array([[qk, P(1.0, 0.6), P(1.0, -0.6)]], F32)
    if kind == "rot_shared_edge":
        return np.array([[P(0, -1), P(0, 1), P(1, 0)], [P(0, 1), P(0, -1), P(-1, 0)]], F32)
    if kind == "rot_hub":
        n = 5 + i % 3
        ang = (np.arange(n) + 0.37 * (i % 5)) * (2 * np.pi / n)
        ring = [P(np.cos(u), np.sin(u)) for u in ang]
        return np.array([[qk, ring[j], ring[(j + 1) % n]] for j in range(n)], F32)
    if kind == "rot_pair":
        one = [P(-1, -0.6), P(1, -0.6), P(0, 1)]
        return np.array([one, one], F32)
    if kind == "rot_far":
        return np.array([[P(-3, -2), P(3, -2), P(0, 3)]], F32)      # narrower than the probe spacing: the parallel rays of the other probes pass it
    raise KeyError(kind)


def ddgi_rot_case(raygen, name, counts, R, orientation, seed, all_hit=None, all_miss=None, in_plane=None):
    """a rotation (or a scaled one) as orientation: every ray has its own direction and its own construct 1.5 .. 3.5 away from its probe
    (probes are 8 apart).  all_hit: a probe inside a closed octahedron; all_miss: a probe without constructs; in_plane: a probe inside a
    triangle of the plane z == its z."""
    ddgi = _grid(counts, R, lo=(1.0, -2.0, 0.5))
    c = _new_case(name, ddgi, orientation, raygen)
    rays = c["rays"]
    tris, n_tris, facing = [], 0, []
    for p in range(rays.shape[0]):
        o = rays[p, 0, 0:3]
        if p == all_miss:
            _mark(c, (p, slice(None)), "all_miss")
            continue
        if p == all_hit:
            r = 0.5
            ax = [np.asarray(v, np.float64) * r for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
            t = np.array([[o + sx * ax[0], o + sy * ax[1], o + sz * ax[2]] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]).astype(F32)
            _mark(c, (p, slice(None)), "all_hit", 0, (n_tris, len(t)))
            tris.append(t); n_tris += len(t)
            facing.append(o.astype(np.float64)[None] - t.astype(np.float64).mean(1))      # inwards: the probe sees the inside
            continue
        for r in range(rays.shape[1]):
            i = p * rays.shape[1] + r + seed
            kind = ROT_KINDS[i % len(ROT_KINDS)]
            k = ULPS[(i // len(ROT_KINDS)) % len(ULPS)]
            dist = 9000.0 if kind == "rot_far" else 1.5 + 0.5 * (i % 5)
            t = rot_construct(kind, o, rays[p, r, 4:7], dist, k, i, size=0.15 if kind != "rot_far" else 1.0)
            _mark(c, (p, r), kind, k, (n_tris, len(t)))
            c["tdist"][p, r] = dist
            tris.append(t); n_tris += len(t)
            facing.append(np.tile(-rays[p, r, 4:7].astype(np.float64), (len(t), 1)))
        if p == in_plane:
            tris.append(np.array([[(o[0] - 1.0, o[1] - 1.0, o[2]), (o[0] + 1.0, o[1] - 1.0, o[2]), (o[0], o[1] + 1.0, o[2])]], F32))
            facing.append(np.zeros((1, 3)))
            n_tris += 1
    c["knife"] = {"rot_vertex": "hit"}
    c["must_hit"] = ("rot_shared_edge", "rot_hub", "rot_pair", "all_hit")
    tris = np.concatenate(tris)
    if all_miss is not None:
        # a triangle whose bounding sphere touches a ray of the all-miss probe collapses to a point (its index stays): that probe sees nothing
        v = tris.astype(np.float64)
        ctr = v.mean(1)
        rad = np.linalg.norm(v - ctr[:, None], axis=2).max(1) + 0.01
        o, dd = rays[all_miss, :, 0:3].astype(np.float64), rays[all_miss, :, 4:7].astype(np.float64)
        rel = ctr[:, None, :] - o[None]
        along = np.clip((rel * dd[None]).sum(2), 0.0, 10000.0)
        near = (np.linalg.norm(rel - along[..., None] * dd[None], axis=2) <= rad[:, None]).any(1)
        tris[near] = tris[near][:, 0:1, :]
        c["collapsed"] = int(near.sum())
        for idx in np.flatnonzero(near):      # the rays whose construct lost a triangle leave their family
            _mark(c, (c["own"][..., 0] <= idx) & (idx < c["own"][..., 0] + c["own"][..., 1]), "collapsed", 0, (-1, -1))
    c["sd"] = scene_of(tris, name, facing=np.concatenate(facing))
    return c


def ddgi_box_plane_case(raygen, child_boxes, name="box_planes", seed=7):
    """a soup only; the grid starts ON child-box planes of its BVH in x, y and z (probe 0 lies on three planes, its neighbours along each axis on
    two) and the orientation is diag(0,0,1): rays run in face planes and along box edges"""
    rng = np.random.RandomState(seed)
    soup = np.concatenate([tc.background(rng, (0.0, 0.0, 0.0), (20.0, 20.0, 12.0), 6000, 0.8), tc.background(rng, (0.0, 0.0, 0.0), (20.0, 20.0, 12.0), 30, 4.0)])
    soup[::5, :, 2] = np.round(soup[::5, :, 2] * 2.0) / 2.0
    soup = soup.astype(F32)
    boxes = child_boxes(soup)
    wide = boxes[(boxes["hi"][:, 0] - boxes["lo"][:, 0] > 2.0) & (boxes["depth"] >= 1)]
    b = wide[len(wide) // 2]
    start = (b["lo"][0], b["lo"][1], b["lo"][2])
    counts, R = (2, 3, 2), 64
    ddgi = synth_env.ddgi_uniforms(start, tuple(float(s) + 6.0 for s in start), probe_counts=counts, rays_per_probe=R, normal_bias=0.1)
    ddgi["grid_start_position"] = start
    c = _new_case(name, ddgi, DIAG_Z, raygen)
    _mark(c, np.ones(c["family"].shape, bool), "graze")
    c["sd"] = scene_of(soup, name)
    c["box"] = b
    return c


DDGI_FAMILIES = ("tmin", "tmax") + AXIS_KINDS + ("rot_vertex", "rot_shared_edge", "rot_hub", "rot_pair", "rot_far", "all_hit", "all_miss", "graze")


def ddgi_cases(raygen, child_boxes):
    """raygen(ddgi, orientation) -> [n_probes][R][8]"""
    out = [ddgi_axis_case(raygen, f"axis_{'x'.join(map(str, counts))}_r{R}", counts, R, v)
           for v, (counts, R) in enumerate((((3, 2, 2), 64), ((2, 3, 2), 100), ((2, 3, 2), 64), ((3, 2, 2), 100)))]
    out.append(ddgi_rot_case(raygen, "rot_r37", (3, 2, 2), 37, rotation(11), 0, all_hit=4, all_miss=11, in_plane=7))
    out.append(ddgi_rot_case(raygen, "rot_r100", (2, 3, 2), 100, rotation(12), 3, all_hit=9, all_miss=0))
    out.append(ddgi_rot_case(raygen, "scaled_r1", (3, 2, 2), 1, rotation(13, 2.5), 1))
    out.append(ddgi_box_plane_case(raygen, child_boxes))
    # the same scenes again as a later frame (infinite bounces read position-coded previous atlases) and as a z-slab shard
    later = Case(out[4]); later.update(name="rot_r37_later", first=False, infinite_bounces=1)
    first_inf = Case(out[5]); first_inf.update(name="rot_r100_first_inf", first=True, infinite_bounces=1)      # the first frame ignores the switch
    shard = Case(out[4]); shard.update(name="rot_r37_shard", shard=(1, 2))
    shard2 = Case(out[1]); shard2.update(name="axis_2x3x2_r100_shard_later", shard=(1, 2), first=False, infinite_bounces=1)
    return out + [later, first_inf, shard, shard2]


# ================================================================================================================ reflections trace
SIZES = ((61, 45), (52, 37))
SKY, MIRROR, GGX, DDGI_ROUGH, NO_THREAD = 0, 1, 2, 3, -1      # raygen's regimes (oracle/pyoracle_reflections.py)
REFL_TILE_SHAPES = ("tile_all_sky", "tile_all_rough", "tile_one_tracer", "tile_full", "tile_one_rough", "tile_one_tracer_among_rough", "tile_ragged_edge_only")


def padded8(w, h):
    return ((h + 7) // 8) * 8, ((w + 7) // 8) * 8


def roughness_codes():
    """fp16 roughness values at the regime thresholds: the two codes to either side of 0.05 (0.05 itself is no fp16 value: its nearest code lies
    below it) and of 0.75 (an fp16 value: 0.75 itself is GGX, one code up is rough) -> (values around 0.05, values around 0.75), float16"""
    a, b = np.float16(0.05), np.float16(0.75)
    dn, up = (lambda v: np.nextafter(v, np.float16(-1))), (lambda v: np.nextafter(v, np.float16(2)))
    return np.array([dn(a), a, up(a), up(up(a))], np.float16), np.array([dn(b), b, up(b), up(up(b))], np.float16)


def refl_params(**kw):
    p = dict(bias=0.5, trim=0.8, num_frames=0, sample_gi=1, approximate_with_ddgi=1, gi_intensity=0.5, rough_ddgi_intensity=0.5, ibl_indirect_specular_intensity=0.05)
    p.update(kw)
    return p


def coded_env(cube=4, pre_size=4, pre_levels=3, lut_size=8):
    """sky / prefiltered chain / BRDF LUT whose texels carry their position, all small (a hit's specular term stays far under the 0.7 clamp)"""
    sky = coded_sky(cube)
    pre = np.concatenate([(f16(coded_sky(pre_size >> l)) * F32(0.5 + 0.1 * l)).astype(np.float16).view(np.uint16).reshape(-1) for l in range(pre_levels)])
    y, x = np.mgrid[0:lut_size, 0:lut_size]
    lut = half(np.stack([0.2 + 0.05 * x / lut_size, 0.05 + 0.05 * y / lut_size], -1))
    return dict(sky=sky, prefiltered=np.ascontiguousarray(pre), pre_size=pre_size, pre_levels=pre_levels, lut=np.ascontiguousarray(lut))


class RFrame(dict):
    def of(self, name):
        return self["family"] == self["names"].index(name)

    def label(self, y, x):
        return self["names"][int(self["family"][y, x])]


def _rframe(name, w, h, scale, translate, cam, params, depth=0.25, rough=0.0, code=(0.0, 0.0)):
    ph, pw = padded8(w, h)
    gb2, gb3 = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 4), np.uint16)
    gb2[..., 0], gb2[..., 1] = half(code[0]), half(code[1])
    gb3[..., 0] = half(rough)
    ubo = tc.affine_ubo(scale, translate, light((0.3, 0.5, -0.8)))      # from below: the mirror rays run upwards and their constructs face down, towards them
    ubo["cam_pos"][0:3] = cam
    return RFrame(name=name, w=w, h=h, depth=np.full((h, w), depth, F32), gb2=gb2, gb3=gb3, ubo=ubo, params=params, family=np.zeros((ph, pw), np.int16),
                  names=["plain"], ulps=np.zeros((ph, pw), np.int16), own=np.full((ph, pw, 2), -1, np.int32), tdist=np.zeros((ph, pw), F32), knife={}, must_hit=())


def _variant(f, name, **params):
    g = RFrame(f)
    p = dict(f["params"]); p.update(params)
    g.update(name=name, params=p, knife={}, aimed=False)
    return g


def _tile(tx, ty):
    return np.s_[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]


def refl_tiles_group(raygen, seed=20):
    """61x45, the camera 2000 above the middle of a plane z = 4 of normals (0,0,1), bias 0.5: every mirror ray runs upwards, a degree or two off
    +z, each with its own direction.
      tile row 0   the tile shapes: all sky / all DDGI-rough (no ray in the wave) / one tracing lane / 64 tracing lanes / one rough lane among 63
                   tracers / one tracer among 63 rough lanes (both exercise the single gather site); tile 6: the regime ties (roughness at the
                   fp16 codes around 0.05 and 0.75); tile column 7 and tile row 5 are ragged: their off-image lanes serve the walk; in tiles
                   (7, 2) and (2, 5) only the image's last column / row has geometry
      below        one construct across every pixel's ray (vertex at fl(o + t d) stepped by ulps, shared edge, closed fan, the same triangle
                   twice, a far triangle), each triangle with a material of its own (metallic 0 / 0.5 / 1 cycling)
    Frames over the same triangles: approximate_with_ddgi 0 with sample_gi 0, trim 0 and trim 1 (the GGX rays move; nothing is aimed at them)."""
    w, h = SIZES[0]
    f = _rframe("tiles", w, h, (32.0, 24.0, 16.0), (40.0, 30.0, 0.0), (40.0, 30.0, 2000.0), refl_params())
    d, g3 = f["depth"], f["gb3"]
    ph, pw = padded8(w, h)
    fam = lambda sel, name, **kw: _mark(f, sel, name, **kw)
    d[_tile(0, 0)] = 1.0; fam(_tile(0, 0), "tile_all_sky")
    g3[_tile(1, 0)][..., 0] = half(0.9); fam(_tile(1, 0), "tile_all_rough")
    d[_tile(2, 0)] = 1.0; d[3, 16 + 5] = 0.25; fam(_tile(2, 0), "tile_one_tracer")
    fam(_tile(3, 0), "tile_full")
    g3[2, 32 + 6, 0] = half(0.9); fam(_tile(4, 0), "tile_one_rough")
    g3[_tile(5, 0)][..., 0] = half(0.9); g3[5, 40 + 1, 0] = half(0.0); fam(_tile(5, 0), "tile_one_tracer_among_rough")
    lo, hi = roughness_codes()
    codes = np.concatenate([lo, hi])
    for i in range(64):
        g3[i // 8, 48 + i % 8, 0] = codes[(i + i // 8) % len(codes)].view(np.uint16)
    fam(_tile(6, 0), "regime_ties")
    # rows 1 ..: roughness 0 (mirror) and, every third pixel, 0.3 (GGX); every eleventh the codes at the thresholds again
    body = np.zeros((ph, pw), bool)
    body[8:h, 0:w] = True
    ys, xs = np.nonzero(body)
    for i, (y, x) in enumerate(zip(ys, xs)):
        if i % 3 == 1:
            g3[y, x, 0] = half(0.3)
        if i % 11 == 5:
            g3[y, x, 0] = codes[(i // 11) % len(codes)].view(np.uint16)
    ragged = np.zeros((ph, pw), bool)
    ragged[:, 56:] = True; ragged[40:, :] = True
    # two ragged tiles in which ONLY the image's last column / last row has geometry: a few tracing lanes, sky lanes and no-thread lanes in one wave
    d[_tile(7, 2)][:, 0:4] = 1.0; fam(_tile(7, 2), "tile_ragged_edge_only")
    d[40:44, 16:24] = 1.0; fam(_tile(2, 5), "tile_ragged_edge_only")
    rays = raygen(f)
    assert ((rays[..., 3] == NO_THREAD) == ~np.pad(np.ones((h, w), bool), ((0, ph - h), (0, pw - w)))).all()
    tris, n_tris, facing = [], 0, []
    targets = [(y, x) for y, x in zip(*np.nonzero((rays[..., 7] != 0)))]
    for i, (y, x) in enumerate(targets):
        row0 = y < 8
        kind = ROT_KINDS[(i + 2 * y) % len(ROT_KINDS)] if not (row0 and f.label(y, x) == "regime_ties") else "rot_pair"
        k = ULPS[(i // len(ROT_KINDS) + y) % len(ULPS)]
        dist = 9000.0 if kind == "rot_far" else 2.0 + 0.5 * ((x + 2 * y) % 5)
        t = rot_construct(kind, rays[y, x, 0:3], rays[y, x, 4:7], dist, k, i, size=0.15 if kind != "rot_far" else 0.1)
        if not row0 and f.label(y, x) != "tile_ragged_edge_only":
            fam((y, x), kind + ("_ragged" if ragged[y, x] else ""), ulps=k)
        f["ulps"][y, x] = k
        f["own"][y, x] = (n_tris, len(t))
        f["tdist"][y, x] = dist
        tris.append(t); n_tris += len(t)
        facing.append(np.tile(-rays[y, x, 4:7].astype(np.float64), (len(t), 1)))
    f["knife"] = {"rot_vertex": "hit", "rot_vertex_ragged": "hit", "regime_ties": "regime"}
    f["must_hit"] = ("rot_shared_edge", "rot_hub", "rot_pair", "rot_shared_edge_ragged", "rot_hub_ragged", "rot_pair_ragged")
    f["aimed"] = True
    frames = [f, _variant(f, "tiles_approx0_gi0", approximate_with_ddgi=0, sample_gi=0), _variant(f, "tiles_trim0", trim=0.0), _variant(f, "tiles_trim1", trim=1.0, approximate_with_ddgi=0)]
    frames[1]["knife"] = {"regime_ties": "regime"}
    return dict(name="tiles", sd=scene_of(np.concatenate(tris), "refl_tiles", facing=np.concatenate(facing)), frames=frames)


def refl_interval_group(raygen, seed=21):
    """52x37, bias 0, depth 0 (and -0): every origin has z == 0 exactly; the camera stands 600 above pixel (26, 18), whose Wo is exactly (0,0,1)
    (N.Wo == 1).  Per pixel a cover at z = fl(t d.z), t around t_min = 0.001 and t_max = 10000 by ulps, or at t ~ 2 (plain).  Set-up oddities in the
    first rows: depth nextafter(1, 0), values above 1, the NU oct code (a normal an ulp longer than 1), normals across (N.Wo ~ 0) and away from the
    camera (N = (0,0,-1): the mirror ray starts in the surface it leaves), GGX at roughness 0.05-and-an-ulp and 1.0."""
    import filter_cases as fcs
    w, h = SIZES[1]
    f = _rframe("interval", w, h, (26.0, 18.5, 16.0), (30.0, 20.0, 0.0), (0.0, 0.0, 0.0), refl_params(bias=0.0, approximate_with_ddgi=0), depth=0.0)
    f["depth"][::3, ::2] = -0.0
    ph, pw = padded8(w, h)
    d, g2, g3 = f["depth"], f["gb2"], f["gb3"]
    nu = dict((n, (a, b)) for n, a, b in fcs.NORMALS)
    odd = [("depth_below_one", dict(depth=np.nextafter(F32(1), F32(0)))), ("depth_above_one", dict(depth=F32(1.5))), ("depth_three", dict(depth=F32(3.0))),
           ("normal_NU", dict(code=nu["NU"])), ("normal_across", dict(code=nu["+X"])), ("normal_away", dict(code=nu["-Z"])),
           ("ggx_rough_min", dict(rough=np.nextafter(np.float16(0.05), np.float16(1)))), ("ggx_rough_one", dict(rough=np.float16(1.0)))]
    for x in range(w):
        name, kw = odd[x % len(odd)]
        for y in (0, 1):
            if "depth" in kw:
                d[y, x] = kw["depth"]
            if "code" in kw:
                g2[y, x, 0], g2[y, x, 1] = kw["code"]
            if "rough" in kw:
                g3[y, x, 0] = np.float16(kw["rough"]).view(np.uint16)
            _mark(f, (y, x), name)
    rays0 = raygen(f)
    f["ubo"]["cam_pos"][0:3] = rays0[18, 26, 0:3] + F32([0.0, 0.0, 600.0])      # bias 0: the origin is P
    rays = raygen(f)
    assert np.array_equal(rays[18, 26, 4:7], F32([0, 0, 1])) and (rays[2:h, :w, 2] == 0).all()
    kinds = ("tmin", "tmax", "plain", "tmin")
    tris, n_tris, facing = [], 0, []
    for y in range(2, h):
        for x in range(w):
            i = y * w + x
            kind, k = kinds[(i + y) % 4], ULPS[(i // 4 + y) % len(ULPS)]
            o, dr = rays[y, x, 0:3], rays[y, x, 4:7]
            t = {"tmin": rc.step_ulps(F32(0.001), k)[()], "tmax": rc.step_ulps(F32(10000.0), k)[()], "plain": F32(2.0)}[kind]
            q = (o.astype(np.float64) + float(t) * dr.astype(np.float64))
            c = tc.cover(F32([q[0], q[1], 0.0]), F32(F32(t) * dr[2]), s=0.25 if kind != "tmax" else 2.0, flip=bool(x % 2))
            _mark(f, (y, x), kind, k, (n_tris, len(c)))
            tris.append(c); n_tris += len(c)
            facing.append(np.tile(-dr.astype(np.float64), (len(c), 1)))
    f["knife"] = {"tmin": "hit", "tmax": "hit"}
    f["aimed"] = True
    return dict(name="interval", sd=scene_of(np.concatenate(tris), "refl_interval", facing=np.concatenate(facing)), frames=[f, _variant(f, "interval_gi1_approx1", sample_gi=1, approximate_with_ddgi=1)])


ODDITIES = ("depth_below_one", "depth_above_one", "depth_three", "normal_NU", "normal_across", "normal_away", "ggx_rough_min", "ggx_rough_one")


def refl_seams_group(raygen, closest, seed=22):
    """52x37, bias 0, normals (0,0,1), equal pixel pitch in x and y, P.z = 16 * depth exactly; ONE triangle set, three frames.
      sky_seams    the camera at z == 0 in the surface's plane, rows 0 .. 11, negative depths: a pixel's depth is -|dx| / 16 (or -|dy| / 16, whichever
                   is larger), so that cam - P has z == |x| (or |y|) EXACTLY; normalising keeps the equality and the mirror direction of N = (0,0,1)
                   is (-Wo.x, -Wo.y, Wo.z): a MISS whose direction lies exactly on the seam between a side face and the +Z face of the sky cube — and,
                   with the depth one fp32 ulp up / down, just to either side of it.  Nothing lies above these rows.
      sky_seams_xy the same idea for the seam between two SIDE faces: a view_proj_inverse whose y row takes the depth, so that |d.x| == |d.y| > |d.z|
      length_ties  the camera 600 above pixel (26, 28), rows 20 .. 36, depth 0: per pixel a cover whose height is SEARCHED (17 candidates an ulp apart,
                   each evaluated by `closest`, the brute-force query) until the hit's 0.001f + t is exactly the midpoint of two fp16 values near 1
                   (the stored ray_length rounds to the even one) or one fp32 ulp beside it
      oddities     the same camera, rows 12 .. 19: the ray set-up oddities of the interval frame, each with the same triangle twice across its ray
                   (a HIT, equal t), and with trim 0 and trim 1 (frames oddities_trim0 / _trim1: the GGX rays at roughness 0.05-and-a-code and 1.0 move)"""
    import filter_cases as fcs
    w, h = SIZES[1]
    scale, translate = (26.0, 18.5, 16.0), (30.0, 20.0, 0.0)
    base = _rframe("probe", w, h, scale, translate, (0.0, 0.0, 0.0), refl_params(bias=0.0, approximate_with_ddgi=0), depth=0.0)
    P = raygen(base)[..., 0:3]                                              # bias 0: the origin is P
    ph, pw = padded8(w, h)
    # ---- sky seams
    s = _rframe("sky_seams", w, h, scale, translate, (0.0, 0.0, 0.0), refl_params(bias=0.0, approximate_with_ddgi=0), depth=1.0)
    cam = F32([P[11, 26, 0], P[11, 26, 1], 0.0])        # in the last seam row: every seam ray runs away from the rows below, over nothing
    s["ubo"]["cam_pos"][0:3] = cam
    for y in range(12):
        for x in range(w):
            dx, dy = np.abs(F32(cam[0] - P[y, x, 0])), np.abs(F32(cam[1] - P[y, x, 1]))
            m = max(dx, dy)
            if m == 0:
                continue
            k = (0, 0, 1, -1)[(x + 3 * y) % 4]
            s["depth"][y, x] = rc.step_ulps(F32(-m / F32(16.0)), k)[()]
            _mark(s, (y, x), "sky_seam" if k == 0 else "sky_seam_beside", k)
    s["aimed"] = True
    # ---- the seam between two SIDE faces: an affine view_proj_inverse whose y row takes the depth (P = (26 ndc_x + 30, 16 depth, 18.5 ndc_y - 100)),
    # so that the depth sets cam.y - P.y = |dx| exactly: |d.x| == |d.y| > |d.z|.  The surface lies 100 below everything and the rays leave towards -y.
    s2 = _rframe("sky_seams_xy", w, h, scale, translate, (0.0, 0.0, 0.0), refl_params(bias=0.0, approximate_with_ddgi=0), depth=1.0)
    m = np.zeros((4, 4), F32)
    m[0, 0], m[0, 3], m[1, 2], m[2, 1], m[2, 3], m[3, 3] = scale[0], translate[0], 16.0, scale[1], -100.0, 1.0
    s2["ubo"]["view_proj_inverse"] = m.T.reshape(16)
    s2["depth"][0:12] = 0.0
    P2 = raygen(s2)[..., 0:3]
    cam2 = F32([P2[6, 26, 0], 0.0, P2[6, 26, 2]])
    s2["ubo"]["cam_pos"][0:3] = cam2
    s2["depth"][0:12] = 1.0
    for y in range(12):
        for x in range(w):
            dx, dz = np.abs(F32(cam2[0] - P2[y, x, 0])), np.abs(F32(cam2[2] - P2[y, x, 2]))
            if dx <= dz:
                continue
            k = (0, 0, 1, -1)[(x + 3 * y) % 4]
            s2["depth"][y, x] = rc.step_ulps(F32(-dx / F32(16.0)), k)[()]
            _mark(s2, (y, x), "sky_seam_xy" if k == 0 else "sky_seam_xy_beside", k)
    s2["aimed"] = True
    # ---- length ties and oddities
    f = _rframe("length_ties", w, h, scale, translate, tuple(P[28, 26] + F32([0.0, 0.0, 600.0])), refl_params(bias=0.0, approximate_with_ddgi=0), depth=1.0)
    f["depth"][12:h] = 0.0
    d, g2, g3 = f["depth"], f["gb2"], f["gb3"]
    nu = dict((n, (a, b)) for n, a, b in fcs.NORMALS)
    odd = dict(depth_below_one=dict(depth=np.nextafter(F32(1), F32(0))), depth_above_one=dict(depth=F32(1.5)), depth_three=dict(depth=F32(3.0)),
               normal_NU=dict(code=nu["NU"]), normal_across=dict(code=nu["+X"]), normal_away=dict(code=nu["-Z"]),
               ggx_rough_min=dict(rough=np.nextafter(np.float16(0.05), np.float16(1))), ggx_rough_one=dict(rough=np.float16(1.0)))
    for y in range(12, 20):
        for x in range(w):
            name = ODDITIES[(x + y) % len(ODDITIES)]
            kw = odd[name]
            if (x + y) % 3 == 0 or y % 2:          # spaced out: a third of the even rows
                d[y, x] = 1.0
                continue
            if "depth" in kw:
                d[y, x] = kw["depth"]
            if "code" in kw:
                g2[y, x, 0], g2[y, x, 1] = kw["code"]
            if "rough" in kw:
                g3[y, x, 0] = np.float16(kw["rough"]).view(np.uint16)
            _mark(f, (y, x), name + "_hit")
    rays = raygen(f)
    assert np.array_equal(rays[28, 26, 4:7], F32([0, 0, 1])) and (rays[20:h, :w, 2] == 0).all()
    tris, n_tris, facing = [], 0, []
    for y in range(12, 20):
        for x in range(w):
            if rays[y, x, 7] == 0:
                continue
            t = rot_construct("rot_pair", rays[y, x, 0:3], rays[y, x, 4:7], 2.0, 0, x + y, size=0.12)
            f["own"][y, x], f["tdist"][y, x] = (n_tris, len(t)), 2.0
            tris.append(t); n_tris += len(t)
            facing.append(np.tile(-rays[y, x, 4:7].astype(np.float64), (len(t), 1)))
    ys, xs = np.mgrid[20:h, 0:w]
    ys, xs = ys.ravel(), xs.ravel()
    o, dr = rays[ys, xs, 0:3], rays[ys, xs, 4:7]
    off = np.asarray((0, 0, 1, -1))[(xs + ys) % 4]
    want = np.array([rc.step_ulps(F32(1.0 + ((x + 2 * y) % 6) * 2.0 ** -10 + 2.0 ** -11), int(k))[()] for x, y, k in zip(xs, ys, off)], F32)
    z0 = ((want - F32(0.001)).astype(F32) * dr[:, 2]).astype(F32)
    q = o.astype(np.float64) + dr.astype(np.float64)                       # where the ray is at t == 1
    cover_at = lambda z: np.concatenate([tc.cover(F32([q[i, 0], q[i, 1], 0.0]), z[i], s=0.25, flip=bool(i % 2)) for i in range(len(z))])
    q8 = np.concatenate([o, np.full((len(o), 1), 10000.0, F32), dr, np.full((len(o), 1), 0.001, F32)], 1).astype(F32)
    best = z0.copy()
    found = np.zeros(len(z0), bool)
    for j in sorted(range(-8, 9), key=abs):
        z = rc.step_ulps(z0, np.full(len(z0), j))
        t, prim = closest(cover_at(z), q8)
        ok = ~found & (prim == np.arange(len(z0))) & ((F32(0.001) + t).astype(F32) == want)
        best[ok], found = z[ok], found | ok
    covers = cover_at(best)
    for i, (y, x) in enumerate(zip(ys, xs)):
        _mark(f, (y, x), ("length_tie" if off[i] == 0 else "length_tie_beside") if found[i] else "length_near", int(off[i]), (n_tris + i, 1))
        f["tdist"][y, x] = 1.0
    f["want"] = np.zeros((ph, pw), F32)
    f["want"][ys, xs] = np.where(found, want, 0)
    tris.append(covers); n_tris += len(covers)
    facing.append(-dr.astype(np.float64))
    f["aimed"] = True
    sd = scene_of(np.concatenate(tris), "refl_seams", facing=np.concatenate(facing))
    return dict(name="seams", sd=sd, frames=[s, s2, f, _variant(f, "oddities_trim0", trim=0.0), _variant(f, "oddities_trim1", trim=1.0)])


REFL_FAMILIES = REFL_TILE_SHAPES + ("regime_ties", "rot_vertex", "rot_shared_edge", "rot_hub", "rot_pair", "rot_far", "rot_vertex_ragged", "rot_pair_ragged",
                                    "tmin", "tmax", "sky_seam", "sky_seam_beside", "sky_seam_xy", "sky_seam_xy_beside", "length_tie", "length_tie_beside") + ODDITIES + tuple(n + "_hit" for n in ODDITIES)


def reflection_groups(raygen, closest):
    """raygen(frame) -> [ph][pw][8] (origin, regime, direction, traced); closest(tris, rays [n][8]) -> (t [n], prim [n]) by brute force"""
    return [refl_tiles_group(raygen), refl_interval_group(raygen), refl_seams_group(raygen, closest)]


def refl_ddgi(sd):
    """the probe grid the reflections' gathers read: (3,2,2) over the scene's box, position-coded atlases"""
    lo, hi = sd.bounds()
    return synth_env.ddgi_uniforms(lo - 1.0, hi + 1.0, probe_counts=(3, 2, 2), rays_per_probe=32, normal_bias=0.1)


# ---------------------------------------------------------------------------------------------------------------- with the oracle
def trace_params(p):
    from oracle import pyoracle_reflections as orf
    return orf.TraceParams(p["bias"], p["trim"], p["num_frames"], int(p["sample_gi"]), int(p["approximate_with_ddgi"]), p["gi_intensity"], p["rough_ddgi_intensity"],
                           p["ibl_indirect_specular_intensity"])


def frame_rays(f):
    from oracle import pyoracle_reflections as orf
    sob, sr = synth.blue_noise_tables()
    return orf.gen_rays(f["ubo"], dict(depth=f["depth"], gb2=f["gb2"], gb3=f["gb3"]), sob, sr, trace_params(f["params"]))


def brute_closest(tris, rays8):
    """(t, prim) of the oracle's brute-force closest hit over a throw-away scene of `tris`"""
    from oracle import pyoracle as po
    tuv, prim = po.Scene(scene_of(tris, "probe")).closest_hit(np.ascontiguousarray(rays8, F32), brute_force=True)
    return tuv[:, 0].copy(), prim


@functools.lru_cache(maxsize=1)
def built_reflections():
    return reflection_groups(frame_rays, brute_closest)


@functools.lru_cache(maxsize=1)
def built_ddgi():
    from hybrid_rendering_amd import api
    from oracle import pyoracle_ddgi as od
    return ddgi_cases(od.gen_rays, api.bvh_child_boxes)
