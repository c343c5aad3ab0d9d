"""Crafted inputs for the spatial filters: the shadows' and the reflections' a-trous iterations, the AO bilateral blur and the 4-tap upsample
(the counterpart of tests/reproject_cases.py for the history reprojection).  Numpy only: no GPU, no oracle import.

craft(w, h) builds a self-consistent G-buffer in the layout helpers.to_cuda takes (depth R32F, gb2 = octahedral normal in .xy, gb3 = roughness in
.x, mesh id in .z, linear z in .w; depth == 1 exactly where gb3.w == -1), a tile-class image, and stage inputs for the three passes.  Rendered
frames never hold what these do: every pixel draws its normal, depth step, roughness and sky flag independently from small palettes of edge values,
so that every (centre, tap) combination of them occurs somewhere, at every border and on both sides of every workgroup seam; tile classes are
injected, so dead tiles sit next to live ones and hold non-zero input texels.  Everything is deterministic from (w, h, seed).

Families (info["family"], FAMILY):
  B  border: non-sky pixels of live tiles within 8 texels of a border (a-trous taps at tap distance 1 / 2 / 4 / 8 leave the image; the blur's taps
     read the pinned out-of-image 0: depth 0, AO 0, the normal decoded from (0, 0) = +z, to which most palette normals have a positive dot)
  T  tile classes: pixels of dead tiles and pixels of live tiles with a dead tile within 8 texels (checkerboard, single live / dead tiles, a dead
     tile column and a dead tile row that cross the 32x8 and 32x16 workgroup seams; one live tile wholly of sky)
  S  sky: isolated sky pixels, a sky row, a sky column and a sky block inside live tiles; a sky texel keeps the normal it drew (often its
     neighbours'); gb3_shadows additionally holds linear z of +0, -0 and -2^-10 (a negative z that is not -1) for the shadows' a-trous
  R  roughness at the fp16 values around 0.05 and 0.75 (reflections)
  W  weights: everything else — the normal palette gives dot exactly 0, -1, 1, and one ulp above 1 (NU: a code whose fp32 decode has
     dot(n, n) > 1); depth steps of 0, one fp16 ulp, 1, 100 and 6e4; value regimes per image quadrant: variance 0 with inputs equal or one fp16 ulp
     apart, variance 0 with arbitrary inputs, small variance, large variance
  U  upsample: craft_upsample()

describe(info, y, x, step, radius) names the pixel's case and its notable taps for failure messages."""
import numpy as np

F32 = np.float32
FAMILY = dict(none=0, B=1, T=2, S=3, R=4, W=5, U=6)
FAMILY_NAME = {v: k for k, v in FAMILY.items()}

# (w, h): one 32x8 region with every step-8 tap outside; whole tiles with five and nine tile columns; ragged in both axes
SHAPES = [(24, 8), (40, 24), (72, 40), (37, 21)]
BAND_SHAPE, BAND_ROWS = (333, 141), (40, 96)

SHADOW_VARIANTS = [dict(), dict(phi_normal=24.0), dict(phi_normal=12.5), dict(radius=2), dict(power=2.0, sigma_depth=0.25)]
AO_RADII = [4, 1, 6]
REFLECTION_VARIANTS = [dict(), dict(radius=2), dict(approximate_with_ddgi=0)]


def f16bits(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def f16val(b):
    return np.asarray(b, np.uint16).view(np.float16).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- normals
def decode32(exb, eyb):
    """octohedral_to_direction (common.glsl:150-156) in float32, operation by operation as the oracle's orc_math.h does it"""
    ex, ey = f16val(exb), f16val(eyb)
    one = F32(1.0)
    z = ((one - np.abs(ex)).astype(F32) - np.abs(ey)).astype(F32)
    sx, sy = np.where(ex >= 0, one, -one).astype(F32), np.where(ey >= 0, one, -one).astype(F32)
    nx = np.where(z < 0, ((one - np.abs(ey)).astype(F32) * sx).astype(F32), ex)
    ny = np.where(z < 0, ((one - np.abs(ex)).astype(F32) * sy).astype(F32), ey)
    v = np.stack([nx, ny, z], -1).astype(F32)
    inv = (one / np.sqrt(dot32(v, v)).astype(F32)).astype(F32)
    return (v * inv[..., None]).astype(F32)


def dot32(a, b):
    return ((a[..., 0] * b[..., 0]).astype(F32) + (a[..., 1] * b[..., 1]).astype(F32) + (a[..., 2] * b[..., 2]).astype(F32)).astype(F32)


def beyond_one_codes(near=(1.0 / 32, 1.0 / 64), reach=48):
    """fp16 oct codes around `near` whose two fp32 decodes give dot(n, n) > 1 (one ulp: the clamp to [0, 1] is what keeps pow() in range),
    searched in float32 the way reproject_cases.normal_candidates searches its knife edge; sorted by distance from `near`"""
    bx, by = int(f16bits(near[0])), int(f16bits(near[1]))
    xs, ys = np.meshgrid(np.arange(bx - reach, bx + reach + 1), np.arange(by - reach, by + reach + 1))
    xb, yb = xs.ravel().astype(np.uint16), ys.ravel().astype(np.uint16)
    n = decode32(xb, yb)
    sel = dot32(n, n) == np.nextafter(F32(1.0), F32(2.0))
    xb, yb = xb[sel], yb[sel]
    order = np.argsort(np.abs(xb.astype(np.int64) - bx) + np.abs(yb.astype(np.int64) - by), kind="stable")
    return xb[order], yb[order]


def _palette():
    ux, uy = beyond_one_codes()
    assert len(ux), "no oct code with dot(n, n) > 1 in float32 near the base normal"
    h = lambda v: int(f16bits(v))
    return [("N0", h(1.0 / 32), h(1.0 / 64)),              # the base normal, 2 degrees off +z
            ("NU", int(ux[0]), int(uy[0])),                 # dot(NU, NU) = 1 + one fp32 ulp
            ("N1", h(0.125), h(-0.0625)),                   # dot(N0, N1) ~ 0.99
            ("+Z", h(0.0), h(0.0)), ("+X", h(1.0), h(0.0)), ("+Y", h(0.0), h(1.0)),     # pairwise dot exactly 0
            ("-Z", h(1.0), h(1.0)), ("-X", h(-1.0), h(0.0))]                                 # dot exactly -1 with +Z / +X


NORMALS = _palette()
NORMAL_P = [0.33, 0.29, 0.10, 0.08, 0.05, 0.04, 0.07, 0.04]
Z_STEPS = [("z", 8.0), ("z+1ulp", 8.0078125), ("z+1", 9.0), ("z+100", 108.0), ("z=6e4", 60000.0)]
Z_P = [0.50, 0.16, 0.16, 0.12, 0.06]
SHADOW_Z = [("+0", 0x0000), ("-0", 0x8000), ("-2^-10", 0x9400)]      # gb3_shadows only: z < 0 passes through, -0 and +0 do not


def _roughness_palette():
    b05, lim = int(f16bits(0.05)), F32(0.05)
    near = [b for b in (b05 - 1, b05, b05 + 1)]
    below = max(b for b in near if f16val(b) < lim)
    above = min(b for b in near if not f16val(b) < lim)
    b75 = int(f16bits(0.75))
    return [("0.4", int(f16bits(0.4))), ("<0.05", below), (">=0.05", above), ("0.75-1ulp", b75 - 1), ("0.75", b75), ("0.75+1ulp", b75 + 1),
            ("0", 0), ("1", int(f16bits(1.0)))]


ROUGHNESS = _roughness_palette()
ROUGHNESS_P = [0.40, 0.11, 0.11, 0.10, 0.10, 0.10, 0.04, 0.04]
REGIMES = ["variance 0, inputs equal or 1 fp16 ulp apart", "variance 0", "small variance", "large variance"]


# ---------------------------------------------------------------------------------------------------------------- tiles
def tile_pattern(tw, th):
    """live (1) / dead (0) 8x8 tiles: left half a checkerboard; a dead tile column at tw // 2 — tile column 4 is the first of the second
    32-pixel workgroup column — and a dead tile row at th // 2 (tile row 2: the seam of the 32x16 regions); right half: a single live tile in dead
    surroundings above the dead row, a single dead tile in live surroundings below it"""
    t = np.ones((th, tw), np.uint8)
    ty, tx = np.mgrid[0:th, 0:tw]
    half = tw // 2
    left = tx < half
    t[left] = ((tx + ty + 1) & 1)[left]
    if tw < 5:
        t[:, 1] = 0
        return t
    t[:, half] = 0
    if th >= 3:
        t[th // 2, :] = 0
        t[:th // 2, half + 1:] = 0
        t[max(th // 2 - 1, 0), min(half + 2, tw - 1)] = 1          # single live tile
        t[th - 1, min(half + 2, tw - 1)] = 0                        # single dead tile
    return t


def per_pixel(tiles, h, w):
    return np.kron(tiles, np.ones((8, 8), tiles.dtype))[:h, :w]


def near_mask(mask, reach):
    """pixels with a True of `mask` within `reach` texels (Chebyshev)"""
    h, w = mask.shape
    out = np.zeros_like(mask)
    pad = np.pad(mask, reach)
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


# ---------------------------------------------------------------------------------------------------------------- the crafted frame
def craft(w, h, seed=0):
    rng = np.random.RandomState((seed * 1000003 + w * 131 + h) & 0x7fffffff)
    th, tw = (h + 7) // 8, (w + 7) // 8
    tiles = tile_pattern(tw, th)
    live = per_pixel(tiles, h, w).astype(bool)
    ys, xs = np.mgrid[0:h, 0:w]
    normal = rng.choice(len(NORMALS), size=(h, w), p=NORMAL_P)
    zstep = rng.choice(len(Z_STEPS), size=(h, w), p=Z_P)
    rough = rng.choice(len(ROUGHNESS), size=(h, w), p=ROUGHNESS_P)
    sky = rng.rand(h, w) < 0.13
    sky[min(5, h - 2), w // 4:w // 4 + 10] = True                      # a sky row
    sky[2:max(h - 2, 3), max(w - 6, 0)] = True                         # a sky column
    sky[h // 2:h // 2 + 3, w // 2 + 1:w // 2 + 4] = True               # a sky block
    lt = np.argwhere(tiles == 1)
    sky_tile = tuple(int(v) for v in lt[len(lt) // 2]) if len(lt) > 2 else None    # one live tile wholly of sky
    if sky_tile is not None:
        sky[sky_tile[0] * 8:sky_tile[0] * 8 + 8, sky_tile[1] * 8:sky_tile[1] * 8 + 8] = True
    shadow_z = np.where(rng.rand(h, w) < 0.18,rng.randint(0, len(SHADOW_Z), (h, w)), -1)
    shadow_z[sky] = -1

    gb2 = np.zeros((h, w, 4), np.uint16)
    gb2[..., 0] = np.array([n[1] for n in NORMALS], np.uint16)[normal]
    gb2[..., 1] = np.array([n[2] for n in NORMALS], np.uint16)[normal]
    zval = np.array([z[1] for z in Z_STEPS], np.float64)[zstep]
    gb3 = np.zeros((h, w, 4), np.uint16)
    gb3[..., 0] = np.array([r[1] for r in ROUGHNESS], np.uint16)[rough]
    gb3[..., 2] = f16bits(7.0)
    gb3[..., 3] = np.where(sky, f16bits(-1.0), f16bits(zval))
    depth = np.where(sky, 1.0, 1.0 - 1.0 / (1.0 + zval)).astype(F32)
    assert ((depth == 1.0) == sky).all() and (depth[~sky] > 0).all()
    gb3_shadows = gb3.copy()
    sel = shadow_z >= 0
    gb3_shadows[..., 3][sel] = np.array([z[1] for z in SHADOW_Z], np.uint16)[shadow_z[sel]]
    gb = dict(gb1=np.zeros((h, w, 4), np.uint8), gb2=gb2, gb3=gb3, depth=depth)

    # ---- stage inputs: a value regime per image quadrant
    regime = (xs >= w // 2) * 2 + (ys >= h // 2)          # quadrants: taps at distance 8 stay inside their regime
    half, ulp = int(f16bits(0.5)), 1
    u = rng.rand(h, w)
    pick = rng.rand(h, w)
    anyv = np.where(pick < 0.2, 0.0, np.where(pick < 0.4, 1.0, u))
    pair = (half + (rng.rand(h, w) < 0.5) * ulp).astype(np.uint16)
    value = np.where(regime == 0, pair, f16bits(anyv)).astype(np.uint16)
    var = np.select([regime <= 1, regime == 2], [0.0, rng.rand(h, w) * 1e-2], 0.25 + rng.rand(h, w) * 3.75)
    shadows_in = np.stack([value, f16bits(var)], -1).astype(np.uint16)
    tiny = rng.rand(h, w) * 2.0 ** -10
    ao_in = np.where(regime == 0, pair, np.where(regime == 2, f16bits(tiny), f16bits(anyv))).astype(np.uint16)
    rgb = np.stack([np.where(regime == 0, pair, f16bits(np.where(pick < 0.2, 0.0, rng.rand(h, w)))) for _ in range(3)], -1)
    refl_in = np.concatenate([rgb, f16bits(var)[..., None]], -1).astype(np.uint16)
    hot = rng.rand(h, w) < 0.06
    refl_hdr = refl_in.copy()
    refl_hdr[..., :3][hot] = f16bits(10.0 ** rng.uniform(3.0, np.log10(6.0e4), (int(hot.sum()), 3)))
    refl_hdr[..., 3][hot] = f16bits(10.0 ** rng.uniform(0.0, np.log10(6.0e4), int(hot.sum())))

    # ---- families
    border = np.minimum(np.minimum(xs, w - 1 - xs), np.minimum(ys, h - 1 - ys))
    fam = np.full((h, w), FAMILY["W"], np.uint8)
    fam[(rough != 0)] = FAMILY["R"]
    fam[(border < 8)] = FAMILY["B"]
    fam[near_mask(~live, 8)] = FAMILY["T"]
    fam[sky | (shadow_z >= 0)] = FAMILY["S"]
    return dict(w=w, h=h, gb=gb, gb3_shadows=gb3_shadows, tiles=tiles, live=live, sky=sky, sky_tile=sky_tile, normal=normal, zstep=zstep, rough=rough,
                shadow_z=shadow_z, regime=regime, family=fam, border=border, shadows_in=shadows_in, ao_in=ao_in, refl_in=refl_in, refl_hdr=refl_hdr)


def shadows_gb(info):
    """the G-buffer of the shadows' a-trous: the consistent one with linear z of +0 / -0 / -2^-10 on the SHADOW_Z pixels"""
    return dict(info["gb"], gb3=info["gb3_shadows"])


def _pixel(info, y, x, shadows=False):
    if not (0 <= y < info["h"] and 0 <= x < info["w"]):
        return "outside the image"
    s = [f"{'live' if info['live'][y, x] else 'dead'} tile ({y >> 3}, {x >> 3})", f"normal {NORMALS[info['normal'][y, x]][0]}"]
    if info["sky"][y, x]:
        s.append("sky")
    elif shadows and info["shadow_z"][y, x] >= 0:
        s.append(f"linear z {SHADOW_Z[info['shadow_z'][y, x]][0]}")
    else:
        s.append(Z_STEPS[info["zstep"][y, x]][0])
    s.append(f"roughness {ROUGHNESS[info['rough'][y, x]][0]}")
    return ", ".join(s)


def describe(info, y, x, step=1, radius=1, direction=None, shadows=False):
    """family, case and the notable taps of pixel (y, x) for a filter with taps at (xx, yy) * step, |xx|, |yy| <= radius (direction: the blur's
    1-D taps i * direction, |i| <= radius)"""
    y, x = int(y), int(x)
    out = [f"({y}, {x}) family {FAMILY_NAME[int(info['family'][y, x])]}: {_pixel(info, y, x, shadows)}, border distance {int(info['border'][y, x])}, "
           f"regime '{REGIMES[int(info['regime'][y, x])]}'"]
    taps = [(i * direction[1], i * direction[0]) for i in range(-radius, radius + 1) if i] if direction is not None else \
           [(yy * step, xx * step) for yy in range(-radius, radius + 1) for xx in range(-radius, radius + 1) if xx or yy]
    notable = []
    for dy, dx in taps:
        ty, tx = y + dy, x + dx
        inside = 0 <= ty < info["h"] and 0 <= tx < info["w"]
        if not inside or not info["live"][ty, tx] or info["sky"][ty, tx] or info["normal"][ty, tx] >= 3 or (shadows and info["shadow_z"][ty, tx] >= 0):
            notable.append(f"tap ({dy:+d}, {dx:+d}): {_pixel(info, ty, tx, shadows)}")
    return "; ".join(out + notable[:6])


# ---------------------------------------------------------------------------------------------------------------- through the temporal stage
def pack_mask(bits, pad=0):
    """bool [h, w] -> the trace stages' mask words [ceil(h / 4), ceil(w / 8)]: bit (y & 3) * 8 + (x & 7) of word (y >> 2, x >> 3); the bits
    of a ragged word that lie outside the image are `pad`"""
    h, w = bits.shape
    p = np.full((((h + 3) // 4) * 4, ((w + 7) // 8) * 8), pad, np.uint32)
    p[:h, :w] = bits
    out = np.zeros((p.shape[0] // 4, p.shape[1] // 8), np.uint32)
    for ly in range(4):
        for lx in range(8):
            out |= p[ly::4, lx::8] << np.uint32(ly * 8 + lx)
    return out


def craft_history(info, seed=0):
    """What the fused launches need, which run only behind the temporal stage: trace outputs and history images that make the temporal stage (static
    camera, previous G-buffer = current) produce the tile pattern of info["tiles"] again with fractional values and non-zero variance everywhere.
    Shadows: a dead tile has no lit pixel and history 0 (few lit pixels around it: the clamp to mean -+ sd / 2 keeps the history at 0 while
    the mean is below 0.2), but non-zero history moments, so its variance is not 0.  AO: a dead tile's AO is 1 everywhere (all rays unoccluded, history
    1, dense bits around it).  Reflections: a dead tile is one whose roughness is below 0.05 on every pixel (gb_reflections).
    The tile that is wholly sky comes out dead from every temporal stage: a live sky tile exists only by injection."""
    h, w, live = info["h"], info["w"], info["live"]
    rng = np.random.RandomState((seed * 92821 + w * 211 + h * 17 + 5) & 0x7fffffff)
    near = near_mask(~live, 8) & live
    r16 = lambda *s: f16bits(rng.rand(*s))
    length = lambda: f16bits(rng.randint(1, 33, (h, w)).astype(np.float64))
    shadow_bits = rng.rand(h, w) < np.where(~live, 0.0, np.where(near, 0.1, 0.5))
    ao_bits = rng.rand(h, w) < np.where(~live, 1.0, np.where(near, 0.95, 0.5))
    m1 = rng.rand(h, w)
    moments = np.stack([f16bits(m1), f16bits(m1 * m1 + rng.rand(h, w) * 0.2), length(), np.zeros((h, w), np.uint16)], -1).astype(np.uint16)
    rim = near_mask(~live, 2)      # the history taps of a dead tile's edge pixels reach their neighbours
    shadows_hist = np.stack([np.where(rim, 0, r16(h, w)), r16(h, w)], -1).astype(np.uint16)
    ao_hist = np.where(rim, f16bits(1.0), r16(h, w)).astype(np.uint16)
    trace = np.concatenate([f16bits(rng.rand(h, w, 3) * 0.7), f16bits(rng.uniform(1.0, 50.0, (h, w, 1)))], -1).astype(np.uint16)
    refl_hist = np.concatenate([r16(h, w, 3), f16bits(rng.rand(h, w, 1) * 0.05)], -1).astype(np.uint16)
    gb3 = info["gb"]["gb3"].copy()
    gb3[..., 0][~live] = 0
    return dict(shadow_mask=pack_mask(shadow_bits), ao_mask=pack_mask(ao_bits, 1)[None], moments=moments, shadows_hist=shadows_hist, ao_hist=ao_hist, ao_len=length(),
                trace=trace, refl_hist=refl_hist, refl_moments=moments.copy(), gb_reflections=dict(info["gb"], gb3=gb3))


def temporal_tiles(info):
    """the tile classes the temporal stages make of craft_history(): info["tiles"] with the wholly-sky tile dead"""
    t = info["tiles"].copy()
    if info["sky_tile"] is not None:
        t[info["sky_tile"]] = 0
    return t


# ---------------------------------------------------------------------------------------------------------------- upsample
UPSAMPLE_LOW = [(20, 12), (18, 10)]
UPSAMPLE_FULL = [(1, 0), (1, 1), (2, 0), (2, 3)]      # (scale, extra): full extent = (low << scale) + extra — the pass's low extent is full >> scale


def craft_upsample(w, h, scale, extra, seed=0):
    """independent full-resolution and low-resolution G-buffers (gb2, gb3) and low-resolution inputs for the 4-tap upsample.
    Full extent (w << scale) + extra: even and odd sizes, so that the clamp to edge decides taps at the first and last column and row.
    Low-resolution sky texels at 35 % in the left half (0 - 4 sky taps per cross), an all-sky block (4 sky taps under non-sky centres); full-resolution
    normals opposite (-Z over +Z) to all four coarse taps in a band of rows (total weight 0 < 1e-8 -> 0 / 1e-8); AO inputs of 0, below 2^-10 and above 1"""
    rng = np.random.RandomState((seed * 7919 + w * 977 + h * 31 + scale * 5 + extra) & 0x7fffffff)
    W, H = (w << scale) + extra, (h << scale) + extra
    hb = lambda v: int(f16bits(v))
    pz, nz = (hb(0.0), hb(0.0)), (hb(1.0), hb(1.0))

    def level(hh, ww, sky, opposite, zjit):
        gb2 = np.zeros((hh, ww, 4), np.uint16)
        n = rng.choice(3, size=(hh, ww), p=[0.6, 0.25, 0.15])
        gb2[..., 0] = np.array([NORMALS[0][1], NORMALS[1][1], NORMALS[3][1]], np.uint16)[n]
        gb2[..., 1] = np.array([NORMALS[0][2], NORMALS[1][2], NORMALS[3][2]], np.uint16)[n]
        gb2[..., 0][opposite], gb2[..., 1][opposite] = nz
        z = 8.0 + zjit * rng.choice([0.0, 0.0078125, 1.0, 100.0], size=(hh, ww), p=[0.5, 0.2, 0.2, 0.1])
        gb3 = np.zeros((hh, ww, 4), np.uint16)
        gb3[..., 0], gb3[..., 2] = hb(0.4), hb(7.0)
        gb3[..., 3] = np.where(sky, hb(-1.0), f16bits(z))
        depth = np.where(sky, 1.0, 1.0 - 1.0 / (1.0 + z)).astype(F32)
        return dict(gb1=np.zeros((hh, ww, 4), np.uint8), gb2=gb2, gb3=gb3, depth=depth)

    ly, lx = np.mgrid[0:h, 0:w]
    low_sky = (rng.rand(h, w) < 0.35) & (lx < w // 2)
    low_sky[h // 2:h // 2 + 4, w // 2 + 1:w // 2 + 7] = True
    low = level(h, w, low_sky, np.zeros((h, w), bool), 1.0)
    low["gb2"][..., 0][(ly >= h - 3) & ~low_sky], low["gb2"][..., 1][(ly >= h - 3) & ~low_sky] = pz     # +Z under the -Z band of the full image
    fy = np.mgrid[0:H, 0:W][0]
    full_sky = rng.rand(H, W) < 0.06
    opposite = (fy >= H - (2 << scale)) & ~full_sky
    full = level(H, W, full_sky, opposite, 1.0)
    regime = (lx * 4 // w)
    u = rng.rand(h, w)
    ao = np.select([regime == 0, regime == 1, regime == 2], [u, u * 2.0 ** -10, 1.0 + u], np.where(u < 0.5, 0.0, u))
    colour = np.stack([rng.rand(h, w), rng.rand(h, w), rng.rand(h, w), rng.rand(h, w) * 0.1], -1)
    fam = np.full((H, W), FAMILY["U"], np.uint8)
    return dict(W=W, H=H, w=w, h=h, scale=scale, full=full, low=low, low_sky=low_sky, full_sky=full_sky, opposite=opposite, family=fam,
                ao_in=f16bits(ao), shadows_in=np.stack([f16bits(u), f16bits(rng.rand(h, w) * 0.1)], -1).astype(np.uint16), refl_in=f16bits(colour))


def upsample_taps(W, H, w, h):
    """[4, H, W, 2] (sy, sx) of the four coarse taps of every full-resolution pixel, float32 as upsample.comp computes them"""
    fy, fx = np.mgrid[0:H, 0:W]
    tu, tv = ((fx.astype(F32) + F32(0.5)) / F32(W)).astype(F32), ((fy.astype(F32) + F32(0.5)) / F32(H)).astype(F32)
    tsx, tsy = (F32(1.0) / F32(w)), (F32(1.0) / F32(h))
    out = []
    for kx, ky in ((0.0, 1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, -1.0)):
        cu, cv = (tu + (F32(kx) * tsx).astype(F32)).astype(F32), (tv + (F32(ky) * tsy).astype(F32)).astype(F32)
        sx = np.clip(np.floor((cu * F32(w)).astype(F32)).astype(np.int64), 0, w - 1)
        sy = np.clip(np.floor((cv * F32(h)).astype(F32)).astype(np.int64), 0, h - 1)
        out.append(np.stack([sy, sx], -1))
    return np.stack(out)


def describe_upsample(info, y, x):
    y, x = int(y), int(x)
    t = upsample_taps(info["W"], info["H"], info["w"], info["h"])[:, y, x]
    taps = ", ".join(f"({int(sy)}, {int(sx)}){' sky' if info['low_sky'][sy, sx] else ''}" for sy, sx in t)
    return (f"({y}, {x}) family U, full {info['W']}x{info['H']} over {info['w']}x{info['h']}: {'sky centre' if info['full_sky'][y, x] else 'surface'}"
            f"{', normal opposite to the coarse taps' if info['opposite'][y, x] else ''}; coarse taps {taps}")
