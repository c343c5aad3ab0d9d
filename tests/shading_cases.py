"""Constructed inputs for the device shading layer (numpy only: no GPU, no oracle) — the counterpart of ray_cases.py and reproject_cases.py for
shading.h, cutout.h and sampling.h, evaluated through hr_selftest_shading (csrc/selftest_shading.h has the modes and the element layout) and its
mirror orc_selftest_shading.

cases(mode) returns a list of Case: one family of elements over one set of tables.  Every mode has a random `bulk` family per table set and the
named edge families of the knife edges a scene reaches only by accident.  A family whose discrete outcome is a TIE carries the expected value in
`expect` (plane -> array), written down by the documented priority and not derived from any implementation.  Tables are tiny and carry their own
coordinates: a cube texel holds (face, iy, ix), a prefiltered texel (8 * level + face, iy, ix), a LUT texel (ix, iy) — so a fetch returns WHERE it
read.  Everything is seeded; nothing here depends on the oracle."""
import functools
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
N_IN = 24
(RNG, CUBE, TEXTURE, BRDF_TERMS, BRDF_UBER, LOBES, LIGHT_HARD, LIGHT_SHADOW, GI_OCT, GI_COORDS, GATHER, SURFACE) = range(12)
MODE_NAMES = ["rng", "cube", "texture", "brdf_terms", "brdf_uber", "lobes", "light_hard", "light_shadow", "gi_oct", "gi_coords", "gather", "surface"]
NOUT = {RNG: 8, CUBE: 8, TEXTURE: 5, BRDF_TERMS: 8, BRDF_UBER: 6, LOBES: 12, LIGHT_HARD: 11, LIGHT_SHADOW: 5, GI_OCT: 11, GI_COORDS: 7, GATHER: 11, SURFACE: 11}
BULK = 4096          # elements of a random family
INT_MAX = 2 ** 31 - 1


@dataclass
class Case:
    mode: int
    family: str
    tables: dict                 # name -> array / int (oracle.pyoracle.shading_tables); tables["key"] names the set
    inp: np.ndarray              # [n][24] float32
    expect: dict = field(default_factory=dict)   # output plane -> expected float32 array (tie families)
    note: str = ""

    @property
    def nout(self):
        return NOUT[self.mode]

    @property
    def name(self):
        return f"{MODE_NAMES[self.mode]}/{self.tables.get('key', '-')}/{self.family}"


def elems(n):
    return np.zeros((n, N_IN), F32)


def up(x, k=1):
    """x moved k fp32 ulps toward +inf (k < 0: toward -inf)"""
    x = np.asarray(x, F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def ladder(x, ks=(-2, -1, 0, 1, 2)):
    return np.array([up(x, k) for k in ks], F32).reshape(-1)


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def unit(v):
    """fp32 normalisation the simple way (the inputs need not be exactly unit: the functions under test normalise where the shaders do)"""
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def rand_unit(rng, n):
    return unit(rng.normal(size=(n, 3)))


# ---------------------------------------------------------------------------------------------------------------------- rng
def cases_rng():
    rng = np.random.RandomState(101)
    v = elems(BULK)
    v[:, 0:3].view(np.uint32)[:] = rng.randint(0, 2 ** 32, size=(BULK, 3), dtype=np.uint64).astype(np.uint32)
    out = [Case(RNG, "bulk", dict(key="none"), v)]
    # pixel coordinates as the passes use them (idx << 16 | idy), frame counters, and the words whose hash or shift loses bits
    words = np.array([0, 1, 2, 0xffff, 0x10000, 0x10001, 0x7fffffff, 0x80000000, 0xffffffff, 61, 0x3d, 0x27d4eb2d, 1919, 1079], np.uint32)
    g = np.array(np.meshgrid(words, words, words[:6], indexing="ij")).reshape(3, -1).T
    e = elems(len(g))
    e[:, 0:3].view(np.uint32)[:] = g
    out.append(Case(RNG, "edge_words", dict(key="none"), e))
    return out


# ---------------------------------------------------------------------------------------------------------------------- cube
@functools.lru_cache(maxsize=None)
def cube_tables(S, pre_size, pre_levels, lut_size):
    def cube(s, tag):
        t = np.zeros((6, s, s, 4), np.float64)
        t[..., 0] = np.arange(6)[:, None, None] + tag
        t[..., 1] = np.arange(s)[None, :, None]
        t[..., 2] = np.arange(s)[None, None, :]
        t[..., 3] = 1.0
        return f16(t)
    pre = np.concatenate([cube(pre_size >> l, 8 * l).reshape(-1) for l in range(pre_levels)])
    lut = np.zeros((lut_size, lut_size, 2), np.float64)
    lut[..., 0] = np.arange(lut_size)[None, :]
    lut[..., 1] = np.arange(lut_size)[:, None]
    return dict(key=f"cube{S}_pre{pre_size}x{pre_levels}_lut{lut_size}", cube=np.ascontiguousarray(cube(S, 0)), cube_size=S, prefiltered=np.ascontiguousarray(pre),
                pre_size=pre_size, pre_levels=pre_levels, lut=np.ascontiguousarray(f16(lut)), lut_size=lut_size)


CUBE_SETS = [(1, 4, 3, 1), (2, 8, 4, 16), (5, 4, 3, 16), (16, 8, 4, 1)]
AXES = [(0, 1), (1, 2), (0, 2)]   # the axis pairs of an edge tie


def face_by_priority(d):
    """Vulkan's face selection with the pinned tie rule: x over y over z, `>=`"""
    ax, ay, az = np.abs(d[..., 0]), np.abs(d[..., 1]), np.abs(d[..., 2])
    fx = np.where(d[..., 0] >= 0, 0, 1)
    fy = np.where(d[..., 1] >= 0, 2, 3)
    fz = np.where(d[..., 2] >= 0, 4, 5)
    return np.where((ax >= ay) & (ax >= az), fx, np.where(ay >= az, fy, fz)).astype(F32)


def cube_edge_dirs():
    """all 12 edge ties (two equal largest components, every sign pair) at two magnitudes and two values of the third component"""
    d = []
    for a, b in AXES:
        c = 3 - a - b
        for sa in (1, -1):
            for sb in (1, -1):
                for m, third in ((1.0, 0.3), (0.3, -0.1), (F32(1e-3), F32(0.0))):      # the third component keeps s, t off texel borders
                    v = np.zeros(3, F32)
                    v[a], v[b], v[c] = sa * m, sb * m, third
                    d.append(v)
    return np.array(d, F32)


def cube_corner_dirs():
    return np.array([[sx * m, sy * m, sz * m] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1) for m in (1.0, 0.7, 3e-5)], F32)


def cube_neighbour_dirs():
    """one ulp to either side of every edge tie: the first component of the pair moved up / down by an ulp in magnitude"""
    base = cube_edge_dirs()
    out, side = [], []
    for v in base:
        big = np.argsort(-np.abs(v), kind="stable")[:2]
        for comp in big:
            for k in (-1, 1):
                w = v.copy()
                w[comp] = np.sign(w[comp]) * up(np.abs(w[comp]), k)
                out.append(w)
                side.append(k)
    return np.array(out, F32), np.array(side)


def cases_cube():
    out = []
    for si, (S, ps, pl, ls) in enumerate(CUBE_SETS):
        T = cube_tables(S, ps, pl, ls)
        rng = np.random.RandomState(200 + si)

        def with_defaults(d, lod=None, u=None, v=None):
            e = elems(len(d))
            e[:, 0:3] = d
            e[:, 3] = rng.uniform(-1.0, pl + 0.5, len(d)) if lod is None else lod
            e[:, 4] = rng.uniform(-0.2, 1.2, len(d)) if u is None else u
            e[:, 5] = rng.uniform(-0.2, 1.2, len(d)) if v is None else v
            return e
        out.append(Case(CUBE, "bulk", T, with_defaults(rng.normal(size=(BULK, 3)).astype(F32))))
        ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
        faces = np.concatenate([ax, ax * F32(1e-20), ax + F32(0.1) * np.roll(ax, 1, 1), ax * F32(3e30)])
        out.append(Case(CUBE, "faces", T, with_defaults(faces), expect={0: face_by_priority(faces)}))
        ed = cube_edge_dirs()
        out.append(Case(CUBE, "edge_ties", T, with_defaults(ed), expect={0: face_by_priority(ed)}, note="ax == ay, ay == az or ax == az: x over y over z"))
        co = cube_corner_dirs()
        out.append(Case(CUBE, "corner_ties", T, with_defaults(co), expect={0: face_by_priority(co)}, note="all three equal: the x face"))
        nb, _ = cube_neighbour_dirs()
        out.append(Case(CUBE, "tie_neighbours", T, with_defaults(nb)))
        # sc / ma == +-1 puts s on 0 or 1: s * S == S takes the upper clamp, -0 and 0 the first texel
        rim = np.array([[1, 1, 1], [1, -1, -1], [1, 1, -1], [1, -1, 1], [1, 0, 0], [1, -0.0, -0.0], [1, up(F32(1), -1), up(F32(-1), 1)]], F32)
        out.append(Case(CUBE, "face_rim", T, with_defaults(rim)))
        degenerate = np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [np.inf, 1, 1], [np.nan, 1, 1], [1, np.nan, 0], [np.inf, np.inf, np.inf]], F32)
        out.append(Case(CUBE, "degenerate_directions", T, with_defaults(degenerate), note="0 / 0 and inf / inf: the texel index comes from a NaN (-> 0)"))
        # the prefiltered chain between two levels: lod + 0.5 on an integer, and an ulp to either side; below the first and past the last level
        lods = np.concatenate([ladder(F32(k + 0.5)) for k in range(-2, pl + 1)] + [np.array([-0.0, 0.0, -1e9, 1e9, 3e9, -3e9, np.inf, -np.inf, np.nan], F32)])
        level = np.floor((lods + F32(0.5)).astype(F32))          # the fp32 sum, as the shader forms it
        level = np.where(np.isnan(level), 0, np.clip(level, 0, pl - 1)).astype(F32)
        dd = np.tile(np.array([[0.3, -0.2, 1.0]], F32), (len(lods), 1))
        out.append(Case(CUBE, "level_ties", T, with_defaults(dd, lod=lods), expect={3: level * 8 + 4},
                        note="floor(fl32(lod + 0.5)) clamped to the chain (NaN: level 0); direction on the +z face"))
        # the LUT at its edges
        us = np.concatenate([np.array([0.0, -0.0, 1.0, up(F32(1), -1), up(F32(1), 1), -1e-30, -0.25, 1.5, 1e9, -1e9, 3e9, -3e9, 1e30, -1e30, np.inf, -np.inf, np.nan], F32),
                             (np.arange(0, ls + 1) / ls).astype(F32), up((np.arange(1, ls + 1) / ls).astype(F32), -1)])
        uu, vv = [a.reshape(-1) for a in np.meshgrid(us, us, indexing="ij")]
        dd = np.tile(np.array([[1.0, 0.11, 0.23]], F32), (len(uu), 1))

        def lut_index(x):
            t = np.floor((x * F32(ls)).astype(F32))
            return (np.where(np.isnan(t), 0, np.clip(t, 0, ls - 1)) + 0.0).astype(F32)      # + 0.0: an index, never -0
        out.append(Case(CUBE, "lut_edges", T, with_defaults(dd, u=uu, v=vv), expect={6: lut_index(uu), 7: lut_index(vv)},
                        note="u == 1 and beyond clamp to the last texel, u < 0 to the first, |u * size| >= 2^31 saturates, NaN -> texel 0"))
    return out


# ---------------------------------------------------------------------------------------------------------------------- texture
TEX_SIZES = [(1, 1), (2, 3), (5, 7), (8, 8)]


@functools.lru_cache(maxsize=None)
def texture_tables():
    rng = np.random.RandomState(300)
    table, data, off = [], [], 0
    for w, h in TEX_SIZES:
        t = rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
        table.append([off, w, h, 0])
        data.append(t.reshape(-1, 4))
        off += w * h
    data = np.concatenate(data)
    data[sum(w * h for w, h in TEX_SIZES[:2]) + 2 * 5 + 3, 3] = 128      # texture 2 (5 x 7), texel (3, 2): alpha 128 / 255, the cutoff of entries 5 and 6
    # per attribute index: opaque, three cutouts at 0.5, one at 0 (never rejects), one exactly on a texel's alpha, one an ulp above it, one at 1
    a128 = (F32(128) / F32(255)).astype(F32)
    tab = np.zeros((8, 2), np.uint32)
    cut = [(0, 0.0), (1, 0.5), (2, 0.5), (3, 0.5), (4, 0.0), (3, a128), (3, up(a128, 1)), (4, 1.0)]
    for q, (tex1, c) in enumerate(cut):
        tab[q] = (tex1, np.asarray(c, F32).reshape(1).view(np.uint32)[0] if tex1 else 0)
    uvs = rng.uniform(-1.5, 2.5, size=(8, 3, 2)).astype(F32)
    centre = np.array([(3 + 0.5) / 5, (2 + 0.5) / 7], F32)          # texel (3, 2) of the 5 x 7 texture
    uvs[5] = centre
    uvs[6] = centre
    return dict(key="tex_1x1_2x3_5x7_8x8", tex_table=np.array(table, np.uint32), tex_data=np.ascontiguousarray(data).view(np.uint32).reshape(-1), cutout_tab=tab,
                uvs=np.ascontiguousarray(uvs), n_tex=len(TEX_SIZES), n_attr=8)


def texture_edge_coords(w):
    """uv = 0, 1, negative, k + 0.5 / w, the texel centres and borders of two periods to either side, each with its ulp neighbours"""
    ks = np.arange(-2, 3)
    base = [0.0, -0.0, 1.0, -1.0, 0.5 / w, 1 - 0.5 / w] + [k + 0.5 / w for k in ks] + [(i + 0.5) / w for i in range(-w - 1, 2 * w + 1)] + [i / w for i in range(-w, 2 * w + 1)]
    base = np.array(base, F32)
    return np.unique(np.concatenate([base, up(base, 1), up(base, -1)]).view(np.uint32)).view(F32)


# (nothing so large that u * extent overflows fp32: inf stands for that, and a float64 restatement would not overflow with it)
OUT_OF_RANGE = np.array([3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 + 256, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)


def cases_texture():
    T = texture_tables()
    rng = np.random.RandomState(301)
    v = elems(BULK)
    v[:, 0] = rng.randint(0, 4, BULK)
    v[:, 1:3] = rng.uniform(-3, 3, size=(BULK, 2))
    v[:, 3] = rng.choice([0, 1, 2, 3, 4, 7], BULK)      # entries 5 and 6 sit on a tie by construction: their family is cutoff_on_a_texel
    b = rng.uniform(0, 1, size=(BULK, 2))
    b[b.sum(1) > 1] = 1 - b[b.sum(1) > 1]
    v[:, 4:6] = b
    out = [Case(TEXTURE, "bulk", T, v)]
    for t, (w, h) in enumerate(TEX_SIZES):
        cu, cv = texture_edge_coords(w), texture_edge_coords(h)
        uu, vv = [a.reshape(-1) for a in np.meshgrid(cu, cv[::3], indexing="ij")]
        u2, v2 = [a.reshape(-1) for a in np.meshgrid(cu[::3], cv, indexing="ij")]
        e = elems(len(uu) + len(u2))
        e[:, 0] = t
        e[:, 1] = np.concatenate([uu, u2])
        e[:, 2] = np.concatenate([vv, v2])
        out.append(Case(TEXTURE, f"edges_{w}x{h}", T, e, note="uv on 0, 1, negative, k + 0.5 / w; wraps both axes both ways"))
        # a coordinate whose texel index leaves the int range: the index saturates (NaN: 0), the neighbour wraps AFTER that.  u * w is an integer
        # there, so both weights on that axis are 1 and 0 and the result is the texel itself
        oo = np.concatenate([OUT_OF_RANGE, (F32(2.0 ** 31) / F32(w)).reshape(1), (F32(-2.0 ** 31) / F32(w)).reshape(1)]).astype(F32)
        uu, vv = [a.reshape(-1) for a in np.meshgrid(oo, np.array([0.3, -3e9, 1e30, np.nan], F32), indexing="ij")]
        e = elems(2 * len(uu))
        e[:, 0] = t
        e[:, 1] = np.concatenate([uu, vv])
        e[:, 2] = np.concatenate([vv, uu])
        out.append(Case(TEXTURE, f"beyond_int_range_{w}x{h}", T, e))
    # the alpha test on a cutoff that a texel's alpha equals exactly: all three uvs are the texel's centre, and the barycentrics are those whose
    # interpolation (c * b0 + c * u) + c * v gives c back without a rounding, so the sample IS the texel (both weights 1 and 0)
    e = elems(16)
    e[:, 3] = np.repeat([5, 6], 8)
    e[:, 4:6] = np.tile(np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.5, 0], [0, 0.5], [-0.0, 1], [1, -0.0]], F32), (2, 1))
    out.append(Case(TEXTURE, "cutoff_on_a_texel", T, e, expect={4: np.repeat([1.0, 0.0], 8).astype(F32)}, note="alpha == cutoff is accepted (rejected iff alpha < cutoff)"))
    e = elems(6 * 7)
    e[:, 3] = np.repeat([0, 1, 2, 3, 4, 7], 7)
    e[:, 4:6] = np.tile(np.array([[0, 0], [1, 0], [0, 1], [-0.0, 1], [0.5, 0.5], [1.5, -0.25], [np.nan, 0]], F32), (6, 1))
    out.append(Case(TEXTURE, "cutout_corners", T, e))
    return out


# ---------------------------------------------------------------------------------------------------------------------- brdf
def brdf_elements(N, Wo, Wi, F0, diffuse, rough, dots=None):
    n = len(N)
    e = elems(n)
    e[:, 0:3], e[:, 3:6], e[:, 6:9] = N, Wo, Wi
    s = (np.asarray(Wo, F32) + np.asarray(Wi, F32)).astype(F32)
    with np.errstate(all="ignore"):
        inv = (F32(1) / np.sqrt(((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]).astype(F32) + s[:, 2] * s[:, 2]).astype(F32))).astype(F32)
        e[:, 9:12] = s * inv[:, None]          # Wh = normalize(Wo + Wi) as the callers form it; Wo == -Wi gives normalize(0) = NaN
    e[:, 12:15], e[:, 15:18], e[:, 18] = F0, diffuse, rough
    if dots is None:
        d = lambda a, b: np.maximum((a * b).sum(1), 0).astype(F32)
        dots = np.stack([d(N, e[:, 9:12]), d(N, Wi), d(N, Wo), d(Wi, e[:, 9:12])], 1)
    e[:, 19:23] = dots
    return e


DOT_EDGES = np.array([0.0, -0.0, 1e-30, 1e-8, 2.5e-5, 1e-4, 1e-3, 0.5, up(F32(1), -1), 1.0], F32)
ROUGH_EDGES = np.array([0.1, up(F32(0.1), 1), 0.0, 1e-3, 0.05, 1.0], F32)


def cases_brdf(mode):
    rng = np.random.RandomState(400)
    n = BULK
    N = rand_unit(rng, n)
    hemi = lambda: unit(rng.normal(size=(n, 3)) * 0.6 + N * 1.0)
    e = brdf_elements(N, hemi(), hemi(), rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3)), rng.uniform(0.1, 1.0, n))
    e[:, 19:23] = rng.uniform(0, 1, (n, 4))      # the terms' dots are independent inputs
    T = dict(key="none")
    out = [Case(mode, "bulk", T, e)]
    # every dot on 0 and the other clamp regions, at the roughness floor and below it
    g = np.array(np.meshgrid(DOT_EDGES, DOT_EDGES, DOT_EDGES[[0, 3, 7, 9]], ROUGH_EDGES, indexing="ij")).reshape(4, -1).T.astype(F32)
    m = len(g)
    e = brdf_elements(np.tile([[0, 0, 1]], (m, 1)), np.tile([[0, 0, 1]], (m, 1)), np.tile([[0, 0, 1]], (m, 1)), np.tile([[0.04, 0.5, 1.0]], (m, 1)),
                      np.tile([[0.8, 0.2, 0.0]], (m, 1)), g[:, 3], dots=np.stack([g[:, 2], g[:, 0], g[:, 1], g[:, 2]], 1))
    out.append(Case(mode, "dots_at_zero", T, e, note="NdotL, NdotV, VdotH, NdotH on 0 / -0 / tiny / 1; roughness 0.1, an ulp above, 0"))
    if mode == BRDF_UBER:
        # grazing geometry through the whole BRDF: Wi or Wo in the tangent plane (NdotL / NdotV exactly 0), below it, and Wo == -Wi (Wh = normalize(0))
        Nn = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8]], F32)
        tang = np.array([[1, 0, 0], [0, 1, 0], [0.8, 0, -0.6]], F32)
        rows = []
        for nn, tt in zip(Nn, tang):
            for r in ROUGH_EDGES[[0, 2, 5]]:
                rows += [(nn, nn, tt, r), (nn, tt, nn, r), (nn, tt, tt, r), (nn, nn, -nn, r), (nn, tt, -tt, r), (nn, -nn, -nn, r), (nn, nn, nn, r)]
        e = brdf_elements(np.array([r[0] for r in rows], F32), np.array([r[1] for r in rows], F32), np.array([r[2] for r in rows], F32),
                          np.tile([[0.04, 0.04, 0.04]], (len(rows), 1)), np.tile([[0.5, 0.5, 0.5]], (len(rows), 1)), np.array([r[3] for r in rows], F32))
        opposite = np.array([np.array_equal(r[1], -r[2]) for r in rows])
        out.append(Case(mode, "grazing", T, e[~opposite], note="NdotL or NdotV exactly 0, or negative"))
        out.append(Case(mode, "wo_opposes_wi", T, e[opposite], note="Wh = normalize(0): NaN"))
    return out


# ---------------------------------------------------------------------------------------------------------------------- lobes
def lobe_elements(N, rx, ry, rough):
    e = elems(len(N))
    e[:, 0:3], e[:, 3], e[:, 4], e[:, 5] = N, rx, ry, rough
    return e


def threshold_normals():
    """N on either side of and on the two basis thresholds: |N.y| > 0.99 (make_rotation_matrix) and |N.z| < 0.999 (importance_sample_ggx).
    dot(N, (0, 1, 0)) is N.y exactly, so the component itself carries the ladder; the rest of N keeps it near unit length."""
    out, side, which = [], [], []
    for thr, comp in ((F32(0.99), 1), (F32(0.999), 2)):
        for sign in (1, -1):
            for k in (-2, -1, 0, 1, 2):
                c = up(thr, k)
                rest = np.sqrt(max(1.0 - float(c) ** 2, 0.0))
                for other in ((rest, 0.0), (0.0, rest), (rest * 0.6, rest * 0.8)):
                    v = np.zeros(3, F32)
                    v[comp] = sign * c
                    v[[i for i in range(3) if i != comp]] = other
                    out.append(v); side.append(k); which.append(comp)
    return np.array(out, F32), np.array(side), np.array(which)


def cases_lobes():
    rng = np.random.RandomState(500)
    T = dict(key="none")
    n = BULK
    # a quarter of the random numbers log-uniform down to 1e-7: next_float returns any multiple of 2^-23, and sin_theta = sqrt(1 - cos_theta^2)
    # cancels for a small one — the bulk has to see what the formula does there
    r0, r1 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    r0[: n // 4], r1[n // 8: n // 4 + n // 8] = 10.0 ** rng.uniform(-7, 0, n // 4), 10.0 ** rng.uniform(-7, 0, n // 4)
    out = [Case(LOBES, "bulk", T, lobe_elements(rand_unit(rng, n), r0, r1, rng.uniform(0.05, 1, n)))]
    tn, _, _ = threshold_normals()
    r = np.array([[0.25, 0.5], [0.7, 0.125], [0.9, 0.9]], F32)
    e = lobe_elements(np.repeat(tn, len(r), 0), np.tile(r[:, 0], len(tn)), np.tile(r[:, 1], len(tn)), F32(0.4))
    out.append(Case(LOBES, "basis_thresholds", T, e, note="|N.y| around 0.99, |N.z| around 0.999, both signs"))
    poles = np.array([[0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0], [-0.0, 1, -0.0]], F32)
    e = lobe_elements(np.repeat(poles, len(r), 0), np.tile(r[:, 0], len(poles)), np.tile(r[:, 1], len(poles)), F32(0.4))
    out.append(Case(LOBES, "poles", T, e, note="N on an axis: the reference vector switches, the cross product has exact zeros"))
    # the random numbers on their edges: rx below the 1e-5 clamp, on it, 0, 1 (sin_theta 0); Ey == 1 (cos_theta 0)
    edge = np.array([0.0, -0.0, 1e-7, up(F32(1e-5), -1), 1e-5, up(F32(1e-5), 1), 0.5, up(F32(1), -1), 1.0], F32)
    a, b, rr = [x.reshape(-1) for x in np.meshgrid(edge, edge, np.array([0.05, 0.1, 0.5, 1.0], F32), indexing="ij")]
    nn = np.tile(np.array([[0.36, 0.48, 0.8]], F32), (len(a), 1))
    out.append(Case(LOBES, "random_number_edges", T, lobe_elements(nn, a, b, rr), note="rx under the 1e-5 clamp, Ey == 1, rx == 1"))
    e = lobe_elements(np.tile(np.array([[0.36, 0.48, 0.8]], F32), (4, 1)), np.array([0.3, 0.3, 0.3, 0.3], F32), np.array([1.0, 1.0, 0.5, -1.0], F32), np.array([0.0, 0.0, 0.0, 0.5], F32))
    e[1, 0:3] = 0
    out.append(Case(LOBES, "degenerate", T, e, note="alpha 0 with Ey 1 is 0 / 0; N = 0; a random number below 0 (sqrt of a negative)"))
    return out


# ---------------------------------------------------------------------------------------------------------------------- lights
LIGHT_COLOUR = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.5, 0.25, 0, 0, 0, 0, 0], F32)


def light_elements(P, N, Wo, rxy, data0, data1, typ, cos_outer, cos_inner):
    n = len(P)
    e = elems(n)
    e[:, 0:3], e[:, 3:6], e[:, 6:9], e[:, 9:11] = P, N, Wo, rxy
    e[:, 11:15], e[:, 15:19], e[:, 19], e[:, 20], e[:, 21] = data0, data1, typ, cos_outer, cos_inner
    return e


def cases_lights(mode):
    rng = np.random.RandomState(600)
    T = dict(key="none", light=LIGHT_COLOUR)
    n = BULK
    d0 = np.concatenate([rand_unit(rng, n), rng.uniform(0.5, 50, (n, 1))], 1)
    d1 = np.concatenate([rng.uniform(-20, 20, (n, 3)), rng.uniform(0, 2, (n, 1))], 1)
    co = rng.uniform(0.2, 0.8, n)
    e = light_elements(rng.uniform(-10, 10, (n, 3)), rand_unit(rng, n), rand_unit(rng, n), rng.uniform(0, 1, (n, 2)), d0, d1, rng.randint(0, 3, n), co, co + rng.uniform(0.01, 0.19, n))
    out = [Case(mode, "bulk", T, e)]
    # P on the light: dist == 0 (point and spot; a directional light ignores the position)
    P = np.array([[1, 2, 3], [0, 0, 0], [-4.5, 1e-3, 7]], F32)
    rows = [(p, t) for p in P for t in (0, 1, 2)]
    m = len(rows)
    e = light_elements(np.array([r[0] for r in rows]), np.tile([[0, 1, 0]], (m, 1)), np.tile([[0, 0.6, 0.8]], (m, 1)), np.tile([[0.3, 0.6]], (m, 1)),
                       np.tile([[0.6, 0.8, 0, 10]], (m, 1)), np.concatenate([np.array([r[0] for r in rows]), np.full((m, 1), 0.5)], 1), np.array([r[1] for r in rows]), 0.5, 0.7)
    out.append(Case(mode, "on_the_light", T, e, note="dist == 0: Wi = normalize(0), attenuation 1 / 0"))
    # a spot cone's smoothstep on either end: to_light is along an axis, so Wi is that axis exactly and dot(Wi, ldir) is one component of ldir —
    # the cone cosines sit on it and an ulp to either side.  The shadow variant keeps Wi on the axis with radius 0; its axis is x (y is its singular one)
    axis = np.array([2.0, 0, 0], F32) if mode == LIGHT_SHADOW else np.array([0, 2.0, 0], F32)
    comp = 0 if mode == LIGHT_SHADOW else 1
    rows = []
    for b in (F32(0.5), F32(0.70710678), F32(0.25)):
        ldir = np.array([0.1, 0.1, 0.3], F32)
        ldir[comp] = b
        for k in (-1, 0, 1):
            rows.append((ldir, up(b, k), up(b, k) + F32(0.2)))          # dot on the outer cosine: smoothstep 0
            rows.append((ldir, up(b, k) - F32(0.2), up(b, k)))          # dot on the inner cosine: smoothstep 1
        rows.append((ldir, b, b))                                        # an empty cone: 0 / 0
        rows.append((ldir, b + F32(0.1), b))                             # inverted cone
    m = len(rows)
    nrm = axis / F32(2)
    e = light_elements(np.zeros((m, 3)), np.tile(nrm, (m, 1)), np.tile([[0.6, 0.0, 0.8]], (m, 1)), np.tile([[0.3, 0.6]], (m, 1)),
                       np.concatenate([np.array([r[0] for r in rows]), np.full((m, 1), 3.0)], 1), np.concatenate([np.tile(axis, (m, 1)), np.zeros((m, 1))], 1), 2,
                       np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))
    out.append(Case(mode, "spot_cone_ends", T, e, note="dot(Wi, ldir) on cos(outer) and cos(inner) and an ulp beside; empty and inverted cones"))
    # the surface facing away, edge on, and toward the light: attenuation == 0 and > 0
    Ns = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 1e-20, 1], [0, -0.0, 0]], F32)
    rows = [(nn, t) for nn in Ns for t in (0, 1, 2)]
    m = len(rows)
    e = light_elements(np.zeros((m, 3)), np.array([r[0] for r in rows]), np.tile([[0, 0.6, 0.8]], (m, 1)), np.tile([[0.5, 0.25]], (m, 1)),
                       np.tile([[0, 1, 0, 5]], (m, 1)), np.tile([[0, 4, 0, 0.0]], (m, 1)), np.array([r[1] for r in rows]), 0.5, 0.7)
    if mode == LIGHT_SHADOW:   # its light direction must not be parallel to y (the family below): the same normals against a light along (0.6, 0.8, 0)
        e[:, 11:14], e[:, 15:18], e[:, 18] = [0.6, 0.8, 0], [3, 4, 0], 0.25
        e[:, 3:6] = np.array([r[0] for r in rows])[:, [1, 0, 2]]
    out.append(Case(mode, "facing", T, e, note="dot(N, Wi) <= 0 gives attenuation 0"))
    if mode == LIGHT_SHADOW:
        # light_dir parallel to (0, 1, 0): the tangent is normalize(0)
        rows = [(t, s) for t in (0, 1, 2) for s in (1.0, -1.0)]
        m = len(rows)
        e = light_elements(np.zeros((m, 3)), np.tile([[0, 1, 0]], (m, 1)), np.tile([[0, 0.6, 0.8]], (m, 1)), np.tile([[0.5, 0.25]], (m, 1)),
                           np.array([[0, r[1], 0, 5] for r in rows]), np.array([[0, 3 * r[1], 0, 0.5] for r in rows]), np.array([r[0] for r in rows]), 0.5, 0.7)
        out.append(Case(mode, "light_dir_parallel_to_y", T, e, note="cross(light_dir, (0, 1, 0)) == 0: NaN tangent, NaN Wi"))
    return out


# ---------------------------------------------------------------------------------------------------------------------- DDGI helpers
def ddgi_uniforms(counts, irr_side, dep_side, visibility, start=(-1.0, 0.5, 2.0), step=(1.5, 2.0, 0.75), normal_bias=0.25, energy=0.85):
    u = np.zeros(22, np.int32)
    f = u.view(F32)
    f[0:3], f[3:6] = start, step
    u[6:9] = counts
    f[9:14] = (4.0, 50.0, 0.98, normal_bias, energy)      # max_distance, depth_sharpness, hysteresis, normal_bias, energy_preservation
    cols = counts[0] * counts[1]
    u[14:17] = (irr_side, (irr_side + 2) * cols + 2, (irr_side + 2) * counts[2] + 2)
    u[17:20] = (dep_side, (dep_side + 2) * cols + 2, (dep_side + 2) * counts[2] + 2)
    u[20:22] = (64, visibility)
    return u


GRIDS = [((1, 1, 1), 2, 6), ((3, 1, 2), 6, 16), ((2, 2, 2), 8, 2), ((2, 2, 2), 16, 16)]


@functools.lru_cache(maxsize=None)
def gather_tables(gi, visibility, depth_kind="random", bias=0.25):
    counts, irr_side, dep_side = GRIDS[gi]
    d = ddgi_uniforms(counts, irr_side, dep_side, visibility, normal_bias=bias)
    rng = np.random.RandomState(700 + gi)
    iw, ih, dw, dh = int(d[15]), int(d[16]), int(d[18]), int(d[19])
    irr = np.concatenate([rng.uniform(0, 4, (ih, iw, 3)), np.ones((ih, iw, 1))], 2)
    if depth_kind == "random":
        mean = rng.uniform(0.1, 3, (dh, dw))
        dep = np.stack([mean, mean * mean + rng.uniform(0, 0.5, (dh, dw))], 2)
    else:
        mean, m2 = dict(one=(1.0, 1.5), zero=(0.0, 0.0), m2_below=(2.0, 1.0))[depth_kind]     # constant atlases: the constructed mean / m2 texels
        dep = np.stack([np.full((dh, dw), mean), np.full((dh, dw), m2)], 2)
    return dict(key=f"grid{'x'.join(map(str, counts))}_irr{irr_side}_dep{dep_side}_vis{visibility}_{depth_kind}_bias{bias}", ddgi=d,
                irradiance=np.ascontiguousarray(f16(irr)), depth=np.ascontiguousarray(f16(dep)), counts=counts)


def gather_elements(uv, P, N, Wo):
    e = elems(len(P))
    e[:, 0:2], e[:, 2:5], e[:, 5:8], e[:, 8:11] = uv, P, N, Wo
    return e


def probe_positions(T):
    d = T["ddgi"]
    f = d.view(F32)
    c = d[6:9]
    g = np.array(np.meshgrid(np.arange(c[0]), np.arange(c[1]), np.arange(c[2]), indexing="ij")).reshape(3, -1).T
    return (f[3:6] * g.astype(F32) + f[0:3]).astype(F32)


def cases_gather():
    out = []
    for gi in range(len(GRIDS)):
        for vis in (0, 1):
            T = gather_tables(gi, vis)
            rng = np.random.RandomState(710 + gi * 2 + vis)
            f = T["ddgi"].view(F32)
            lo, ext = f[0:3], f[3:6] * np.maximum(np.array(T["counts"]) - 1, 1)
            n = BULK // 2
            P = (lo + rng.uniform(-0.3, 1.3, (n, 3)) * ext).astype(F32)      # inside the grid and a third of it outside
            out.append(Case(GATHER, "bulk", T, gather_elements(rng.uniform(-0.1, 1.1, (n, 2)), P, rand_unit(rng, n), rand_unit(rng, n))))
            # the bilinear set-up on both clamps of both axes, on texel centres and borders, and beyond the int range
            w = int(T["ddgi"][15])
            cs = np.concatenate([np.array([0.0, -0.0, 1.0, 0.5 / w, 1 - 0.5 / w, up(F32(0.5 / w), -1), -0.3, 1.3], F32), ((np.arange(0, w, max(w // 6, 1)) + 0.5) / w).astype(F32),
                                 OUT_OF_RANGE])
            uu, vv = [a.reshape(-1) for a in np.meshgrid(cs, cs, indexing="ij")]
            m = len(uu)
            out.append(Case(GATHER, "bilinear_edges", T, gather_elements(np.stack([uu, vv], 1), np.tile(P[:1], (m, 1)), np.tile([[0, 0, 1]], (m, 1)), np.tile([[0, 0.6, 0.8]], (m, 1))),
                            note="u, v on 0 and 1 (both clamps), texel centres, and with a texel index beyond the int range"))
            # P on probes, on probe planes, outside the grid on every side, and further out than an int holds
            pp = probe_positions(T)
            planes = np.concatenate([pp + np.array([0.3, 0, 0], F32) * f[3:6], pp + np.array([0, 0.6, 0.2], F32) * f[3:6], up(pp, 1), up(pp, -1)])
            far = np.array([[1e12, 0, 0], [0, -1e12, 0], [3e9 * 1.5, 3e9 * 2, -3e9], [np.inf, 0, 0], [0, np.nan, 0]], F32) + pp[:1]
            outside = np.concatenate([lo - ext * F32(0.5) - 1, lo + ext * F32(1.5) + 1, lo + np.array([-1, 0.5, 2], F32) * ext]).reshape(-1, 3)
            for fam, Ps in (("on_probes_and_planes", np.concatenate([pp, planes])), ("outside_the_grid", outside), ("beyond_int_range", far)):
                m = len(Ps)
                out.append(Case(GATHER, fam, T, gather_elements(np.zeros((m, 2)), Ps, np.tile([[0.48, 0.6, 0.64]], (m, 1)), np.tile([[0, 0.6, 0.8]], (m, 1)))))
            e = gather_elements(np.zeros((3, 2)), np.tile(pp[:1] + F32(0.2), (3, 1)), np.array([[0, 0, 0], [np.nan, 0, 1], [0, 0, 1]], F32), np.array([[0, 0.6, 0.8], [0, 0.6, 0.8], [np.inf, 0, 0]], F32))
            out.append(Case(GATHER, "nan_net", T, e, note="N = 0 or NaN: the irradiance texel coordinate is NaN, the net is NaN and 0.5 is returned"))
    # the visibility test's knife edges, on constant depth atlases and without the normal bias, so that dist is |P - probe| exactly: a 1 x 1 x 1 grid
    # whose probe sits at grid_start; P on the x axis and dist an ulp ladder around the atlas' mean
    for kind, centre in (("one", 1.0), ("zero", 0.0), ("m2_below", 2.0)):
        T = gather_tables(0, 1, kind, 0.0)
        p0 = T["ddgi"].view(F32)[0:3]
        xs = np.concatenate([ladder(F32(max(centre, 0.25)), range(-4, 5)), np.array([0.25, 0.5, 3.0], F32)])
        # p0.x + x is exact for these x (p0.x = -1): P - probe_pos gives x back
        P = np.stack([(p0[0] + xs).astype(F32), np.full(len(xs), p0[1]), np.full(len(xs), p0[2])], 1)
        m = len(P)
        out.append(Case(GATHER, f"visibility_{kind}", T, gather_elements(np.zeros((m, 2)), P, np.tile([[1, 0, 0]], (m, 1)), np.tile([[0, 0.6, 0.8]], (m, 1))),
                        note=dict(one="dist <= mean true and false within an ulp", zero="variance == 0", m2_below="mean^2 > m2")[kind]))
    return out


def cases_gi_oct():
    T = dict(key="grid3x1x2", ddgi=ddgi_uniforms((3, 1, 2), 6, 16, 1))
    rng = np.random.RandomState(800)
    n = BULK
    e = elems(n)
    e[:, 0:3] = rng.normal(size=(n, 3))
    e[:, 3:5] = rng.uniform(-1, 1, (n, 2))
    e[:, 5] = rng.randint(0, 6, n)
    nn = rng.choice([1, 2, 64, 256], n)
    e[:, 6], e[:, 7] = rng.randint(0, 256, n) % nn, nn
    out = [Case(GI_OCT, "bulk", T, e)]
    s = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-30, up(F32(1), -1)], F32)
    g = np.array(np.meshgrid(s, s, s, indexing="ij")).reshape(3, -1).T
    e = elems(len(g))
    e[:, 0:3] = g
    e[:, 3:5] = g[:, 0:2]              # decode on the corners, the fold (|x| + |y| == 1) and the centre
    e[:, 5] = np.arange(len(g)) % 8 - 1      # probe indices, with one below and one above the grid (kept inside by the self test)
    e[:, 6], e[:, 7] = np.arange(len(g)) % 4, np.array([1, 2, 4, 4])[np.arange(len(g)) % 4]
    out.append(Case(GI_OCT, "axes_folds_zero", T, e, note="v.z == +-0 (the fold's branch), the zero vector (1 / 0), the octahedron's corners and fold line"))
    e = elems(6)
    e[:, 6:8] = [[0, 0], [5, 4], [1e9, 64], [-1, 64], [np.nan, 64], [3, np.inf]]
    out.append(Case(GI_OCT, "fibonacci_out_of_range", T, e, note="n == 0, i >= n, i huge"))
    return out


def cases_gi_coords():
    T = dict(key="none")
    rng = np.random.RandomState(900)
    out = []

    def make(extents, n_each, family, note=""):
        rows = []
        for tw, th, side in extents:
            # the probe index row * per_row + col stays below 2^24: the shader's mod(probe_index, per_row) is a float one, exact only up to there
            per_row = (tw - 2) // (side + 2)
            rows_max = min(max((th - 2) // (side + 2), 1), max(2 ** 24 // per_row, 1))
            e = elems(n_each)
            e[:, 0:3] = rng.normal(size=(n_each, 3))
            e[:6, 0:3] = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [-1, 1, -0.0]], F32)
            e[:, 4], e[:, 5], e[:, 6] = tw, th, side
            e[:, 7] = rng.randint(0, min(per_row, 2 ** 24), n_each)
            e[:, 8] = rng.randint(0, rows_max, n_each)
            e[:2, 7], e[:2, 8] = (0, per_row - 1), (rows_max - 1, 0)      # the first cell of the last row, the last cell of the first row
            rows.append(e)
        out.append(Case(GI_COORDS, family, T, np.concatenate(rows), note=note))
    real = [((s + 2) * c + 2, (s + 2) * r + 2, s) for s in (2, 6, 8, 16) for c, r in ((1, 1), (3, 2), (4, 2), (200, 7))]
    make(real, BULK // len(real), "bulk")
    # atlas extents around and above atlas_div_inrange's 3e5 and div_prepare's 1e6: coordinates only, no atlas of that size exists
    make([(300000, 300000, 8), (300001, 18, 16), (18, 300002, 6), (300010, 300010, 2), (299998, 300002, 8)], 256, "extent_above_3e5", "the !inrange branch of div_by_if")
    make([(1000000, 1000000, 8), (1000001, 34, 16), (18, 1000008, 6), (16777216, 16777216, 8), (2 ** 30, 2 ** 30, 16)], 256, "extent_above_1e6", "div_prepare's generic path")
    return out


# ---------------------------------------------------------------------------------------------------------------------- surface
@functools.lru_cache(maxsize=None)
def surface_tables():
    rng = np.random.RandomState(1000)
    tex = texture_tables()
    pos = rng.uniform(-2, 2, (6, 3, 3)).astype(F32)
    pos[3] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]                  # collinear: the cross product is 0 (a zero-area geometric normal)
    nrm = unit(rng.normal(size=(6, 3, 3)))
    nrm[1] = unit(np.array([[0, 0, 1], [0, 0.1, 1], [0.1, 0, 1]]))
    nrm[2] = 0                                                    # vertex normals that interpolate to 0
    tan = unit(rng.normal(size=(6, 3, 3)))
    tan[4] = nrm[4]                                               # tangent parallel to N under a normal map: TBN = (T, T, N) collapses onto one line
    uvs = rng.uniform(-1, 2, (6, 3, 2)).astype(F32)
    tri_material = np.array([0, 1, 0, 0, 2, 1], np.uint32)
    materials = np.array([[0.8, 0.7, 0.6, 0.0, 0.05, 0, 0, 0], [0.5, 0.5, 0.5, 1.0, 0.6, 0, 0, 0], [0.2, 0.9, 0.4, 0.5, 0.1, 0, 0, 0]], F32)   # roughness 0.05: under the 0.1 floor
    mat_tex = np.array([[-1, -1, -1, -1, 0, 0], [2, -1, 3, 3, 1, 2], [1, 2, -1, 0, 0, 3]], np.int32)      # albedo, normal, roughness, metallic texture, channels
    m = np.array([[2, 0, 0, 0], [0, 0.5, 0, 0], [0.3, 0, 3, 0], [1, -2, 0.5, 1]], F32)                     # column-major, non-uniform scale + shear + translation
    T = dict(tex)
    T.update(key="six_triangles", positions=pos, normals=np.ascontiguousarray(nrm), tangents=np.ascontiguousarray(tan), tri_uvs=uvs, tri_material=tri_material,
             materials=materials, mat_tex=mat_tex, inst_m=np.ascontiguousarray(m.reshape(-1)), n_tris=6, n_mats=3)
    return T


def surface_elements(q, bary, flags):
    e = elems(len(q))
    e[:, 0], e[:, 1:3], e[:, 3] = q, bary, flags
    return e


BARY_EDGES = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [1 / 3, 1 / 3], [0.25, 0.5], [-0.0, 1], [1.25, -0.5]], F32)


def cases_surface():
    T = surface_tables()
    rng = np.random.RandomState(1001)
    n = BULK
    b = rng.uniform(0, 1, (n, 2))
    b[b.sum(1) > 1] = 1 - b[b.sum(1) > 1]
    out = [Case(SURFACE, "bulk", T, surface_elements(rng.choice([0, 1, 4, 5], n), b, rng.randint(0, 16, n)))]

    def fam(name, q, flag_list, note):
        rows = [(q, bb, fl) for bb in BARY_EDGES for fl in flag_list]
        out.append(Case(SURFACE, name, T, surface_elements([r[0] for r in rows], np.array([r[1] for r in rows]), [r[2] for r in rows]), note=note))
    fam("vertex_normals", 0, [1, 1 | 4, 1 | 4 | 8], "triangles 0 and 1 interpolate their vertex normals")
    fam("vertex_normals_b", 1, [1, 1 | 4, 1 | 4 | 8], "")
    fam("cross_product", 0, [0, 4, 4 | 8], "no normals: the geometric normal")
    fam("zero_area_normal", 2, [1, 1 | 2, 1 | 4 | 8], "vertex normals that sum to 0: normalize(0)")
    fam("zero_area_triangle", 3, [0, 2], "a collinear triangle without normals: cross product 0")
    fam("normal_map_tangent_parallel", 4, [1 | 4 | 8, 1 | 2 | 4 | 8, 4 | 8], "the (T, T, N) quirk with T parallel to N")
    fam("normal_map_default_tangent", 4, [1 | 4], "no tangents: (1, 0, 0)")
    fam("instance_nonuniform_scale", 5, [1 | 2, 2, 1 | 2 | 4 | 8], "mat3(model) * n under non-uniform scale and shear, renormalised")
    return out


# ----------------------------------------------------------------------------------------------------------------------
_BUILDERS = {RNG: cases_rng, CUBE: cases_cube, TEXTURE: cases_texture, BRDF_TERMS: lambda: cases_brdf(BRDF_TERMS), BRDF_UBER: lambda: cases_brdf(BRDF_UBER),
             LOBES: cases_lobes, LIGHT_HARD: lambda: cases_lights(LIGHT_HARD), LIGHT_SHADOW: lambda: cases_lights(LIGHT_SHADOW), GI_OCT: cases_gi_oct,
             GI_COORDS: cases_gi_coords, GATHER: cases_gather, SURFACE: cases_surface}


@functools.lru_cache(maxsize=None)
def cases(mode):
    cs = _BUILDERS[mode]()
    for c in cs:
        c.inp = np.ascontiguousarray(c.inp, F32)
        assert c.inp.shape[1] == N_IN and 0 < len(c.inp) <= 1 << 17, c.name
    total = sum(len(c.inp) for c in cs)
    assert total <= 1 << 17, (MODE_NAMES[mode], total)        # at most 2^17 elements per mode
    return cs


def family(mode, name, key=None):
    return [c for c in cases(mode) if c.family == name and (key is None or c.tables.get("key") == key)]
