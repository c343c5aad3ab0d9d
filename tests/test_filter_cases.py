"""The crafted filter inputs of tests/filter_cases.py on the CPU: (1) non-vacuity — on the oracle's stage functions every family really takes its
targeted branch on enough pixels, so that tests/test_gpu_filter_edges.py cannot pass by missing them; (2) THE PIN — the oracle's a-trous, blur and
upsample stages against the reference's own shader text on the same inputs, bit for bit (as tests/test_ref_shaders_nonfinite.py does).

Floors: at least 16 pixels per targeted branch, per shape and tap distance.  Recorded exceptions (floor 4): the 24x8 shape (192 pixels, half of them in
dead tiles), where the tap-based branches are counted at tap distances 1 and 2 only (at 4 and 8 most taps leave the image); the single fp16 neighbours of
the roughness thresholds; the three special linear z values of the shadows' G-buffer; the AO blur at radius 1 (two border lines carry its out-of-image
taps); the first and last column and row of the upsample.  Not counted at all: taps into dead tiles for the vertical blur at 24x8 (one tile row).
The floors are conditions on the inputs: if one is missed, the
palettes' probabilities in filter_cases.py change, not the floor."""
import numpy as np
import pytest

import filter_cases as fc
import helpers
from hybrid_rendering_amd import synth
from oracle import pyref

ZBP = np.asarray(synth.z_buffer_params(), np.float32)
_N = fc.decode32(np.array([n[1] for n in fc.NORMALS], np.uint16), np.array([n[2] for n in fc.NORMALS], np.uint16))
NDOT = fc.dot32(_N[:, None, :], _N[None, :, :])      # float32 dot of every palette pair, as the filters compute it
_info = {}


def info_of(w, h):
    if (w, h) not in _info:
        _info[(w, h)] = fc.craft(w, h)
    return _info[(w, h)]


def floor_of(w, h):
    return 4 if (w, h) == (24, 8) else 16


@pytest.fixture(scope="module")
def rh():
    if not pyref.available():
        pytest.skip("neither the reference tree nor a prebuilt oracle/_ref")
    from oracle import ref_harness
    return ref_harness


def _tap(a, dy, dx):
    """a[y + dy, x + dx] with the coordinates clamped, and the mask of taps inside the image"""
    h, w = a.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    ty, tx = ys + dy, xs + dx
    inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
    return a[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)], inside


def square_taps(step, radius):
    return [(yy * step, xx * step) for yy in range(-radius, radius + 1) for xx in range(-radius, radius + 1) if xx or yy]


def atrous_counts(info, gb3, inp, var_channel, sky_centre, taps, filtered):
    """pixels of `filtered` (centres that run the weighted sum) per targeted tap property"""
    keys = ["outside", "dead_nonzero", "sky_tap", "dot0", "dot<0", "dot1", "dot>1", "dz0", "dz_ulp", "dz1", "dz100", "dz6e4", "var0_equal", "var0_ulp"]
    acc = {k: np.zeros(filtered.shape, bool) for k in keys}
    z = fc.f16val(gb3[..., 3])
    nonzero = (inp != 0).reshape(inp.shape[0], inp.shape[1], -1).any(-1)
    var = fc.f16val(inp[..., var_channel])
    var0 = np.ones(filtered.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v, ins = _tap(var, dy, dx)
            var0 &= ~ins | (v == 0)
    val = inp[..., 0].astype(np.int64)
    for dy, dx in taps:
        tn, ins = _tap(info["normal"], dy, dx)
        d = NDOT[info["normal"], tn]
        tl, _ = _tap(info["live"], dy, dx)
        tz, _ = _tap(z, dy, dx)
        tnz, _ = _tap(nonzero, dy, dx)
        tsky, _ = _tap(sky_centre, dy, dx)
        tv, _ = _tap(val, dy, dx)
        dz = np.abs(z - tz)
        acc["outside"] |= ~ins
        acc["dead_nonzero"] |= ins & ~tl & tnz
        acc["sky_tap"] |= ins & tsky & (d > 0)
        acc["dot0"] |= ins & (d == 0)
        acc["dot<0"] |= ins & (d < 0)
        acc["dot1"] |= ins & (d == 1)
        acc["dot>1"] |= ins & (d > 1)
        plain = ins & ~tsky
        acc["dz0"] |= plain & (dz == 0)
        acc["dz_ulp"] |= plain & (dz == np.float32(0.0078125))
        acc["dz1"] |= plain & (dz == 1)
        acc["dz100"] |= plain & (dz == 100)
        acc["dz6e4"] |= plain & (dz > 5e4)
        acc["var0_equal"] |= ins & var0 & (tv == val)
        acc["var0_ulp"] |= ins & var0 & (np.abs(tv - val) == 1)
    return {k: int((v & filtered).sum()) for k, v in acc.items()}


def _require(counts, floor, what, keys=None):
    low = {k: v for k, v in counts.items() if (keys is None or k in keys) and v < floor}
    assert not low, f"{what}: targeted branches on fewer than {floor} pixels: {low} (all: {counts})"


def test_palettes_hold_the_edge_values():
    """dot exactly 0, -1 and 1; NU's two decodes give dot > 1 by one float32 ulp; the roughness codes straddle 0.05 and 0.75"""
    names = [n[0] for n in fc.NORMALS]
    i = names.index
    assert NDOT[i("+Z"), i("+X")] == 0 and NDOT[i("+X"), i("+Y")] == 0 and NDOT[i("+Z"), i("+Y")] == 0
    assert NDOT[i("+Z"), i("-Z")] == -1 and NDOT[i("+X"), i("-X")] == -1 and NDOT[i("+Z"), i("+Z")] == 1
    assert NDOT[i("NU"), i("NU")] == np.nextafter(np.float32(1), np.float32(2))
    assert 0.9 < NDOT[i("N0"), i("N1")] < 1 and NDOT[i("N0"), i("+Z")] > 0.99
    r = {n: fc.f16val(b) for n, b in fc.ROUGHNESS}
    assert r["<0.05"] < np.float32(0.05) <= r[">=0.05"] and int(dict(fc.ROUGHNESS)[">=0.05"]) - int(dict(fc.ROUGHNESS)["<0.05"]) == 1
    assert r["0.75-1ulp"] < r["0.75"] == np.float32(0.75) < r["0.75+1ulp"]


@pytest.mark.parametrize("w,h", fc.SHAPES + [fc.BAND_SHAPE])
def test_gbuffer_is_self_consistent(w, h):
    info = info_of(w, h)
    gb = info["gb"]
    assert np.array_equal(gb["depth"] == 1.0, fc.f16val(gb["gb3"][..., 3]) == -1.0) and np.array_equal(gb["depth"] == 1.0, info["sky"])
    for k in ("shadows_in", "ao_in", "refl_in", "refl_hdr"):
        v = fc.f16val(info[k])
        assert np.isfinite(v).all() and (v >= 0).all(), k
    assert fc.f16val(info["refl_in"]).max() <= 4.0 and fc.f16val(info["refl_hdr"][..., :3]).max() > 3.0e4
    t = info["tiles"]
    assert 0 < t.sum() < t.size and info["live"].any() and (~info["live"]).any()
    text = fc.describe(info, h // 2, w // 2, 2, 1, shadows=True)
    assert "family" in text and "tile" in text


@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_shadows_atrous_takes_every_branch(oracle, w, h):
    info, fl = info_of(w, h), floor_of(w, h)
    gb = fc.shadows_gb(info)
    inp = info["shadows_in"]
    z = fc.f16val(gb["gb3"][..., 3])
    skyc = z < 0
    filtered = info["live"] & ~skyc
    for k, (name, _) in enumerate(fc.SHADOW_Z):      # +0 and -0 are filtered, -2^-10 passes through
        n = int((info["live"] & (info["shadow_z"] == k)).sum())
        assert n >= 4, f"{w}x{h}: {n} live pixels with linear z {name}"
    assert int((info["live"] & skyc & (z != -1)).sum()) >= 4 and int((filtered & (z == 0)).sum()) >= 8
    for prm in fc.SHADOW_VARIANTS:
        radius = prm.get("radius", 1)
        for i in range(4):
            step = 1 << i
            out = oracle.shadows_atrous(inp, gb["gb2"], gb["gb3"], info["tiles"], step, **dict(prm, power=prm.get("power", 1.2) if i == 3 else 0.0))
            what = f"shadows {w}x{h} {prm} tap distance {step}"
            assert np.isfinite(fc.f16val(out)).all(), what
            passed, cleared = info["live"] & skyc, ~info["live"]
            assert np.array_equal(out[passed], inp[passed]) and passed.sum() >= fl, f"{what}: a centre with z < 0 passes through"
            assert not out[cleared].any() and (inp[cleared] != 0).any(-1).sum() >= fl, f"{what}: a dead tile writes 0 over non-zero input"
            assert (out[filtered] != inp[filtered]).any(-1).sum() >= fl, what
            if (w, h) == (24, 8) and step > 2:
                continue
            _require(atrous_counts(info, gb["gb3"], inp, 1, skyc, square_taps(step, radius), filtered), fl, what)


@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_ao_blur_takes_every_branch(oracle, w, h):
    info, fl = info_of(w, h), floor_of(w, h)
    gb, inp = info["gb"], info["ao_in"]
    filtered = info["live"] & ~info["sky"]
    one = int(fc.f16bits(1.0))
    for radius in fc.AO_RADII:
        for direction in ((1, 0), (0, 1)):
            out = oracle.ao_blur(inp, gb["depth"], gb["gb2"], info["tiles"], ZBP, direction, radius)
            what = f"AO blur {w}x{h} radius {radius} direction {direction}"
            dead, skyc = ~info["live"], info["live"] & info["sky"]
            assert (out[dead] == one).all() and (inp[dead] != one).sum() >= fl, f"{what}: a dead tile writes 1"
            assert (out[skyc] == one).all() and (inp[skyc] != one).sum() >= fl, f"{what}: a sky centre writes 1"
            outside, sky_tap, dead_tap = (np.zeros((h, w), bool) for _ in range(3))
            for k in range(-radius, radius + 1):
                if k:
                    ts, ins = _tap(info["sky"], k * direction[1], k * direction[0])
                    tl, _ = _tap(info["live"], k * direction[1], k * direction[0])
                    outside |= ~ins
                    sky_tap |= ins & ts
                    dead_tap |= ins & ~tl
            # an out-of-image tap reads depth 0, AO 0 and the normal decoded from (0, 0) = +z: its weight is gauss * exp(-1 - wZ) * dot(n, +z)^32 > 0
            weighted = outside & filtered & (_N[info["normal"], 2] > 0.5)
            counts = dict(outside_with_weight=int(weighted.sum()), sky_tap=int((sky_tap & filtered).sum()), dead_tap=int((dead_tap & filtered).sum()))
            if (w, h) == (24, 8) and direction == (0, 1):
                counts.pop("dead_tap")       # one tile row: no vertical tap meets another tile
            _require(counts, 4 if radius == 1 else fl, what)
            # the out-of-image taps carry weight: against a blur that SKIPS them (what a bounds-checked kernel would compute) the weighted pixels change
            if weighted.any():
                skipped = _blur_skipping_outside(inp, gb, direction, radius)
                changed = (np.abs(fc.f16val(out) - skipped) > 1e-3) & weighted
                assert changed.sum() >= min(fl, 4), f"{what}: zeroed out-of-image taps change only {int(changed.sum())} pixels against skipped ones"


def _blur_skipping_outside(inp, gb, direction, radius):
    """float64 restatement of the blur with out-of-image taps SKIPPED (what the reference does not do); only for the comparison above"""
    h, w = inp.shape
    ao, depth = fc.f16val(inp).astype(np.float64), gb["depth"].astype(np.float64)
    lin = 1.0 / (ZBP[2] * depth + ZBP[3])
    n = fc.decode32(gb["gb2"][..., 0], gb["gb2"][..., 1]).astype(np.float64)
    total, tw = ao.copy(), np.ones((h, w))
    dev = radius / 1.5
    for k in range(-radius, radius + 1):
        if not k:
            continue
        dy, dx = k * direction[1], k * direction[0]
        ta, ins = _tap(ao, dy, dx)
        tl, _ = _tap(lin, dy, dx)
        tn, _ = _tap(n, dy, dx)
        g = np.exp(-(k * k) / (2 * dev * dev)) / (np.sqrt(2 * np.pi) * dev)
        wz = np.exp(-np.abs(lin - tl))
        wn = np.clip((n * tn).sum(-1), 0, 1) ** 32
        wgt = np.where(ins, g * np.exp(-1.0 - wz) * wn, 0.0)
        total += wgt * ta
        tw += wgt
    return total / np.maximum(tw, 1e-4)


@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_reflections_atrous_takes_every_branch(oracle, w, h):
    from oracle import pyoracle_reflections as orf
    info, fl = info_of(w, h), floor_of(w, h)
    gb = info["gb"]
    rv = fc.f16val(gb["gb3"][..., 0])
    surface = info["live"] & ~info["sky"]
    for k, (name, _) in enumerate(fc.ROUGHNESS):
        n = int((surface & (info["rough"] == k)).sum())
        assert n >= 4 or name in ("0", "1"), f"{w}x{h}: {n} live surface pixels with roughness {name}"
    for inp_name in ("refl_in", "refl_hdr"):
        inp = info[inp_name]
        for prm in fc.REFLECTION_VARIANTS:
            radius, approx = prm.get("radius", 1), prm.get("approximate_with_ddgi", 1)
            through = surface & ((rv < np.float32(0.05)) | ((rv > np.float32(0.75)) if approx else False))
            filtered = surface & ~through
            for i in range(4):
                step = 1 << i
                out = orf.atrous(inp, gb, info["tiles"], step, radius, 10.0, 32.0, 1.0, approx)
                what = f"reflections {inp_name} {w}x{h} {prm} tap distance {step}"
                dead, skyc = ~info["live"], info["live"] & info["sky"]
                assert np.array_equal(out[dead], inp[dead]), f"{what}: a dead tile copies"
                assert not out[skyc].any() and inp[skyc].any(-1).sum() >= fl, f"{what}: a sky centre writes 0"
                assert np.array_equal(out[through], inp[through]) and through.sum() >= fl, f"{what}: roughness pass-through"
                assert (out[filtered] != inp[filtered]).any(-1).sum() >= fl, what
                # the thresholds' neighbours land on their own sides
                names = [n for n, _ in fc.ROUGHNESS]
                for n, filt in (("<0.05", False), (">=0.05", True), ("0.75-1ulp", True), ("0.75", True), ("0.75+1ulp", not approx)):
                    sel = surface & (info["rough"] == names.index(n))
                    assert (filtered[sel] == filt).all(), (what, n)
                if (w, h) == (24, 8) and step > 2:
                    continue
                _require(atrous_counts(info, gb["gb3"], inp, 3, info["sky"], square_taps(step, radius), filtered), fl, what,
                         keys=("outside", "dead_nonzero", "sky_tap", "dot0", "dot<0", "dot1", "dot>1", "dz0", "dz_ulp", "dz1", "dz100", "dz6e4"))


UPSAMPLE_PASSES = [("ao", 1, 1.0, 1.2, "ao_in"), ("shadows", 1, 0.0, 0.0, "shadows_in"), ("reflections", 4, 0.0, 0.0, "refl_in")]


def upsample_cases():
    return [(w, h, s, e) for (w, h) in fc.UPSAMPLE_LOW for (s, e) in fc.UPSAMPLE_FULL]


@pytest.mark.parametrize("w,h,scale,extra", upsample_cases())
def test_upsample_takes_every_branch(oracle, w, h, scale, extra):
    u = fc.craft_upsample(w, h, scale, extra)
    W, H = u["W"], u["H"]
    assert (W >> scale, H >> scale) == (w, h)
    taps = fc.upsample_taps(W, H, w, h)
    nsky = u["low_sky"][taps[..., 0], taps[..., 1]].sum(0)
    surface = ~u["full_sky"]
    what = f"upsample {W}x{H} over {w}x{h}"
    counts = {f"{k}_sky_taps": int((surface & (nsky == k)).sum()) for k in range(5)}
    counts["sky_centre"] = int(u["full_sky"].sum())
    zero_weight = surface & (u["opposite"] | (nsky == 4))
    counts["weight<1e-8"] = int(zero_weight.sum())
    counts["opposite_normals"] = int((surface & u["opposite"] & (nsky < 4)).sum())
    # the clamp to edge decides a tap: first / last column and row
    fy, fx = np.mgrid[0:H, 0:W]
    for name, sel in (("col0", fx == 0), ("col_last", fx == W - 1), ("row0", fy == 0), ("row_last", fy == H - 1)):
        counts[name] = int((surface & sel).sum())
    _require(counts, 16, what, keys=[k for k in counts if not k.startswith(("col", "row"))])
    _require(counts, 4, what)
    for name, ch, sky_value, power, key in UPSAMPLE_PASSES:
        out = oracle.upsample(u["full"], u["low"], u[key] if u[key].ndim == 3 else u[key][..., None], channels=ch, sky_value=sky_value, power=power)
        v = fc.f16val(out)
        assert np.isfinite(v).all(), (what, name)
        assert (v[u["full_sky"]] == sky_value).all() and not v[zero_weight].any(), f"{what} {name}: sky centres write the sky value, total weight 0 gives 0 / 1e-8 = 0"
        if name == "ao":     # power 1.2 on results of 0, below 2^-10 and above 1
            r = v[..., 0][surface]
            _require(dict(zero=int((r == 0).sum()), tiny=int(((r > 0) & (r < 2.0 ** -10)).sum()), above_1=int((r > 1).sum())), 16, f"{what} AO power")


# ------------------------------------------------------------------------------------------------------------------------ through the temporal stage
def static_ubo(w, h):
    cam = synth.cornell_camera(w / h)
    return synth.make_ubo(cam, None, synth.cornell_light())


@pytest.mark.parametrize("w,h", fc.SHAPES[1:])
def test_temporal_stages_reach_the_fused_launches_families(oracle, w, h):
    """craft_history(): the oracle's temporal stages turn the injected masks and history images into the crafted tile pattern, with fractional
    values and non-zero variance — also inside dead shadow tiles"""
    from oracle import pyoracle_reflections as orf
    info = info_of(w, h)
    hist, ubo, gb = fc.craft_history(info), static_ubo(w, h), info["gb"]
    want = fc.temporal_tiles(info)
    dead = ~fc.per_pixel(want, h, w).astype(bool)
    tv, mom, tiles = oracle.shadows_temporal(ubo, hist["shadow_mask"], gb, gb, hist["shadows_hist"], hist["moments"])
    assert np.array_equal(tiles, want), "shadows: tile classes"
    v, var = fc.f16val(tv[..., 0]), fc.f16val(tv[..., 1])
    counts = dict(dead_nonzero_variance=int((dead & ~info["sky"] & (var > 0)).sum()), fractional=int(((v > 0) & (v < 1)).sum()), variance=int((~dead & (var > 0)).sum()),
                  accepted_history=int((fc.f16val(mom[..., 2]) >= 2).sum()))
    _require(counts, 16, f"shadows temporal {w}x{h}")
    out, ln, tiles = oracle.ao_temporal(ubo, hist["ao_mask"], gb, gb, hist["ao_hist"], hist["ao_len"])
    assert np.array_equal(tiles, want), "AO: tile classes"
    a = fc.f16val(out)
    _require(dict(fractional=int(((a > 0) & (a < 1)).sum()), accepted_history=int((fc.f16val(ln) >= 2).sum())), 16, f"AO temporal {w}x{h}")
    gbr = hist["gb_reflections"]
    for approx in (1, 0):
        oc, om, tiles = orf.temporal(ubo, hist["trace"], gbr, gbr, hist["refl_hist"], hist["refl_moments"], (0.0, 0.0, 0.0), 0.01, 0.2, approx)
        assert np.array_equal(tiles, want), "reflections: tile classes"
        _require(dict(variance=int((fc.f16val(oc[..., 3]) > 0).sum()), accepted_history=int((fc.f16val(om[..., 2]) >= 2).sum())), 16, f"reflections temporal {w}x{h}")


# ------------------------------------------------------------------------------------------------------------------------ THE PIN
PIN_SHAPES = [(40, 24), (37, 21)]


@pytest.mark.parametrize("w,h", PIN_SHAPES)
def test_oracle_shadows_atrous_is_the_reference_shader(oracle, rh, w, h):
    info = info_of(w, h)
    gb, inp = fc.shadows_gb(info), info["shadows_in"]
    den, shd = rh.tile_lists(info["tiles"])
    for prm in fc.SHADOW_VARIANTS:
        for i in range(4):
            p = dict(prm, power=prm.get("power", 1.2) if i == 3 else 0.0)
            ref = rh.shadows_atrous(inp, gb, den, shd, 1 << i, **p)
            got = oracle.shadows_atrous(inp, gb["gb2"], gb["gb3"], info["tiles"], 1 << i, **p)
            helpers.assert_bits_equal_nan(got, ref, f"shadows a-trous {w}x{h} {prm} tap distance {1 << i}")


@pytest.mark.parametrize("w,h", PIN_SHAPES)
def test_oracle_ao_blur_is_the_reference_shader(oracle, rh, w, h):
    info = info_of(w, h)
    gb, inp = info["gb"], info["ao_in"]
    den, _ = rh.tile_lists(info["tiles"])
    for radius in fc.AO_RADII:
        for direction in ((1, 0), (0, 1)):
            ref = rh.ao_blur(inp, np.zeros((h, w), np.uint16), gb, den, ZBP, direction, radius, np.full((h, w), 0x3C00, np.uint16))
            got = oracle.ao_blur(inp, gb["depth"], gb["gb2"], info["tiles"], ZBP, direction, radius)
            helpers.assert_bits_equal_nan(got, ref, f"AO blur {w}x{h} radius {radius} direction {direction}")


@pytest.mark.parametrize("w,h", PIN_SHAPES)
def test_oracle_reflections_atrous_is_the_reference_shader(oracle, rh, w, h):
    from oracle import pyoracle_reflections as orf
    info = info_of(w, h)
    gb = info["gb"]
    den, cpy = rh.tile_lists(info["tiles"])
    for inp_name in ("refl_in", "refl_hdr"):
        for prm in fc.REFLECTION_VARIANTS:
            radius, approx = prm.get("radius", 1), prm.get("approximate_with_ddgi", 1)
            for i in range(4):
                ref = rh.reflections_atrous(info[inp_name], gb, den, cpy, 1 << i, radius, 10.0, 32.0, 1.0, approx)
                got = orf.atrous(info[inp_name], gb, info["tiles"], 1 << i, radius, 10.0, 32.0, 1.0, approx)
                helpers.assert_bits_equal_nan(got, ref, f"reflections a-trous {inp_name} {w}x{h} {prm} tap distance {1 << i}")


@pytest.mark.parametrize("w,h,scale,extra", [c for c in upsample_cases() if c[2] == 1])
def test_oracle_upsample_is_the_reference_shader(oracle, rh, w, h, scale, extra):
    """full sizes 40x24, 41x25 (over 20x12) and 36x20, 37x21 (over 18x10): the reference's shader samples mip 1 of the G-buffer, here the crafted low level"""
    u = fc.craft_upsample(w, h, scale, extra)
    for name, ch, sky_value, power, key in UPSAMPLE_PASSES:
        low = u[key]
        ref = rh.upsample(f"{name}/{name}_upsample.comp", [u["full"], u["low"]], 1, low, {1: "r16f", 4: "rgba16f"}[ch], power=power if name == "ao" else None)
        got = oracle.upsample(u["full"], u["low"], low if low.ndim == 3 else low[..., None], channels=ch, sky_value=sky_value, power=power)
        helpers.assert_bits_equal_nan(got, ref, f"{name} upsample {u['W']}x{u['H']} over {w}x{h}")
