"""The spatial filters — the shadows' and the reflections' a-trous kernels, the AO bilateral blur, the 4-tap upsample — on the crafted inputs of
tests/filter_cases.py (families B border, T tile classes, S sky, R roughness, W weights, U upsample), against the oracle's stage functions.  The oracle is
pinned to the reference's shader text on the same inputs, and shown to take every targeted branch, by tests/test_filter_cases.py on the CPU.

Route A, one launch at a time: the pass runs its trace and temporal stage once on the crafted G-buffer (tolerance mode builds its geometry records from
those tensors, which stay alive), then the stage's input image and the tile-class image are overwritten through pass.image() and the stage entry point
is called: atrous_iteration(i) for i = 0..3 (each fed with the crafted input again), blur(0) / blur(1), upsample().
Route B, the fused launches (kf_shadows_atrous01, kf_ao_blur_xy, kf_refl_atrous01), which run only from denoise(): the trace output and the history
images are injected (filter_cases.craft_history), the camera is static with prev == cur, and denoise() runs the temporal stage into them.

exact = 1: every written image equals the oracle's bit for bit, and the rows outside a band stay untouched.  exact = 0: route A answers to
test_gpu_tolerance.compare16 with the arguments that file passes for the same image and no outlier allowance (docs/TOLERANCE.md gives a single launch
none; the tile classes are injected, so no flipped-tile exclusion applies); route B: the fused launches' outputs and feedback copies equal the
unfused chain's (a pass created under HR_FUSE=0) bit for bit, and each launch of that chain answers to the oracle's stage applied to the GPU's own
previous image.  A failing pixel is reported through filter_cases.describe(): family, case and the notable taps."""
import os

import numpy as np
import pytest

import filter_cases as fc
import helpers
from hybrid_rendering_amd import synth, tiling
from test_gpu_tolerance import _key, compare16

pytestmark = pytest.mark.gpu

ZBP = synth.z_buffer_params()
_cache = {}


def _cached(key, make):
    """crafted inputs and oracle results, computed once and shared by the exact and the tolerance test"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _info(w, h):
    return _cached(("info", w, h), lambda: fc.craft(w, h))


def _tables():
    import torch
    sob, sr = synth.blue_noise_tables()
    return torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()


def _ubo(w, h):
    """a static camera: no motion, previous view-projection = current"""
    return synth.make_ubo(synth.cornell_camera(w / h), None, synth.cornell_light())


def _put(view, bits):
    """copy bit patterns into a pass-owned image view (fp16 images as uint16, the mask as uint32, tile classes as uint8)"""
    import torch
    a = np.ascontiguousarray(bits)
    src = torch.from_numpy(a.view({2: np.int16, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]))
    src = src.view(torch.float16) if a.dtype.itemsize == 2 else src
    assert src.numel() == view.numel() and src.dtype == view.dtype, (tuple(src.shape), src.dtype, tuple(view.shape), view.dtype)
    view.copy_(src.reshape(view.shape).cuda())


def _put_tiles(gp, tiles):
    view = gp.image(gp.IMG_TILES)
    assert tuple(view.shape) == tiles.shape, (tuple(view.shape), tiles.shape)
    _put(view, tiles)


def _unfused(make):
    """a pass created with HR_FUSE=0 (developer switch, read once at creation): denoise() launches the stages one by one"""
    old = os.environ.get("HR_FUSE")
    os.environ["HR_FUSE"] = "0"
    try:
        return make()
    finally:
        if old is None:
            del os.environ["HR_FUSE"]
        else:
            os.environ["HR_FUSE"] = old


SENTINEL = 0x3555     # fp16 0.333: what a launch must leave in the rows it does not own


def _check(got, ref, what, exact, tell, rows=None, **rule):
    """got / ref: uint16 images.  exact: bit for bit; else compare16(**rule).  tell(y, x) describes a pixel; rows: the band's rows"""
    got = np.asarray(got).reshape(ref.shape)
    g, r = (got, ref) if rows is None else (got[rows[0]:rows[1]], ref[rows[0]:rows[1]])
    y_off = 0 if rows is None else rows[0]
    if exact:
        bad = (g != r).reshape(g.shape[0], g.shape[1], -1).any(-1)
        if bad.any():
            w = np.argwhere(bad)[:4]
            fl = lambda a, y, x: a[y, x].view(np.float16).astype(np.float32).tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ from the oracle's bit for bit; " +
                                 " | ".join(f"{tell(int(y) + y_off, int(x))}: got {fl(g, y, x)} ref {fl(r, y, x)}" for y, x in w))
        return
    try:
        compare16(g, r, what + " (tolerance mode)", **rule)
    except AssertionError as e:
        d = np.abs(_key(g) - _key(r)).reshape(g.shape[0], g.shape[1], -1).max(-1)
        worst = np.argwhere(d == d.max())[:3]
        raise AssertionError(str(e) + "; worst: " + " | ".join(f"{tell(int(y) + y_off, int(x))} ({int(d[y, x])} ulp)" for y, x in worst)) from None


def _band_args(info, band, history_halo):
    if not band:
        return None, None, (0, info["h"])
    b0, b1 = fc.BAND_ROWS
    return (b0, b1, tiling.HALO, history_halo), (b0, b1), (max(0, b0 - tiling.HALO), min(info["h"], b1 + tiling.HALO))


def _untouched(view_bits, resident, what):
    out = np.concatenate([view_bits[:resident[0]], view_bits[resident[1]:]])
    assert (out == SENTINEL).all(), f"{what}: {int((out != SENTINEL).sum())} values written outside the band's resident rows {resident}"


SHAPE_CASES = [(w, h, False) for (w, h) in fc.SHAPES] + [fc.BAND_SHAPE + (True,)]


# ------------------------------------------------------------------------------------------------------------------------ route A: shadows
@pytest.mark.parametrize("exact,fuse", [(1, True), (0, True), (0, False)], ids=["exact", "tolerance", "tolerance_HR_FUSE0"])
@pytest.mark.parametrize("w,h,band", SHAPE_CASES)
def test_shadows_atrous_iterations(oracle, hr, ctx, w, h, band, exact, fuse):
    """k_shadows_atrous<1 | -1> (exact); kf_shadows_atrous_lds<1 | 2>, kf_shadows_atrous<4 | 8> and the run-time kf_shadows_atrous<0> (radius 2), with
    phi_normal 32 / 24 / 12.5, on linear z of +0, -0, -2^-10 and -1, dead tiles with non-zero input, taps across every border.  A pass created under
    HR_FUSE=0 must launch the same per-iteration kernels (the switch decides what denoise() launches)"""
    import torch
    info = _info(w, h)
    gb, inp = fc.shadows_gb(info), info["shadows_in"]
    gsc = hr.Scene(ctx, helpers.scene_data("cornell"))
    sob_d, sr_d = _tables()
    gb_d = helpers.to_cuda(gb)      # alive until the pass is closed: the geometry records stand for these tensors
    fi = hr.frame_inputs(gb_d, gb_d, _ubo(w, h), 0, 0, sob_d, sr_d)
    bnd, rows, resident = _band_args(info, band, tiling.HISTORY_HALO)
    for prm in (fc.SHADOW_VARIANTS[:1] if band else fc.SHADOW_VARIANTS):
        make = lambda: hr.RayTracedShadows(ctx, w, h, 0, band=bnd)
        gp = make() if fuse else _unfused(make)
        gp.params.exact = exact
        for k, v in prm.items():
            setattr(gp.params, k, v)
        p = gp.params
        try:
            gp.ray_trace(gsc, fi)
            gp.temporal(fi)
            _put_tiles(gp, info["tiles"])
            for i in range(4):
                src, dst = (gp.IMG_TEMPORAL if i == 0 else gp.IMG_ATROUS0 + (i & 1)), gp.IMG_ATROUS0 + ((i & 1) ^ 1)
                _put(gp.image(dst), np.full(inp.shape, SENTINEL, np.uint16))
                _put(gp.image(src), inp)
                gp.atrous_iteration(fi, i)
                torch.cuda.synchronize()
                got = helpers.bits16(gp.image(dst))
                power = p.power if i == 3 else 0.0
                ref = _cached(("shadows", w, h, tuple(sorted(prm.items())), i), lambda: oracle.shadows_atrous(
                    inp, gb["gb2"], gb["gb3"], info["tiles"], 1 << i, p.radius, p.phi_visibility, p.phi_normal, p.sigma_depth, power))
                what = f"shadows a-trous {w}x{h} {prm} iteration {i}"
                tell = lambda y, x: fc.describe(info, y, x, 1 << i, p.radius, shadows=True)
                _check(got, ref, what, exact, tell, rows, variance_channels=(1,))
                if band:
                    _untouched(got.reshape(ref.shape), resident, what)
                if i == p.feedback_iteration:
                    fb = helpers.bits16(gp.image(gp.IMG_PREV)).reshape(ref.shape)
                    assert np.array_equal(fb[resident[0]:resident[1]], got.reshape(ref.shape)[resident[0]:resident[1]]), f"{what}: the feedback copy"
        finally:
            gp.close()
    gsc.close()


# ------------------------------------------------------------------------------------------------------------------------ route A: AO blur
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("w,h,band", SHAPE_CASES)
def test_ao_blur_passes(oracle, hr, ctx, w, h, band, exact):
    """k_ao_blur<4 | -1> (exact), kf_ao_blur / kf_ao_blur_generic (radius 4 / 1 and 6): every tap outside the image reads the pinned 0 — depth 0 through
    linear_eye_depth, AO 0, the normal decoded from (0, 0) — with non-zero weight; sky taps enter with their own depth and normal"""
    import torch
    info = _info(w, h)
    gb, inp = info["gb"], info["ao_in"]
    gsc = hr.Scene(ctx, helpers.scene_data("cornell"))
    sob_d, sr_d = _tables()
    gb_d = helpers.to_cuda(gb)
    fi = hr.frame_inputs(gb_d, gb_d, _ubo(w, h), 0, 0, sob_d, sr_d, z_buffer_params=ZBP)
    bnd, rows, resident = _band_args(info, band, tiling.HALO)
    zb = np.asarray(ZBP, np.float32)
    for radius in (fc.AO_RADII[:1] if band else fc.AO_RADII):
        gp = hr.RayTracedAO(ctx, w, h, 0, band=bnd)
        gp.params.exact, gp.params.blur_radius = exact, radius
        try:
            gp.ray_trace(gsc, fi)
            gp.temporal(fi)
            _put_tiles(gp, info["tiles"])
            for which, direction in ((0, (1, 0)), (1, (0, 1))):
                src, dst = (gp.IMG_AO0 if which == 0 else gp.IMG_BLUR0), (gp.IMG_BLUR0 if which == 0 else gp.IMG_BLUR1)
                _put(gp.image(dst), np.full(inp.shape, SENTINEL, np.uint16))
                _put(gp.image(src), inp)
                gp.blur(fi, which)
                torch.cuda.synchronize()
                got = helpers.bits16(gp.image(dst))
                ref = _cached(("ao", w, h, radius, which), lambda: oracle.ao_blur(inp, gb["depth"], gb["gb2"], info["tiles"], zb, direction, radius))
                what = f"AO blur {w}x{h} radius {radius} pass {which}"
                _check(got, ref, what, exact, lambda y, x: fc.describe(info, y, x, 1, radius, direction=direction), rows)
                if band:
                    _untouched(got.reshape(ref.shape), resident, what)
        finally:
            gp.close()
    gsc.close()


# ------------------------------------------------------------------------------------------------------------------------ route A: reflections
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("w,h,band", SHAPE_CASES)
def test_reflections_atrous_iterations(oracle, hr, ctx, w, h, band, exact):
    """k_refl_atrous<1 | -1> (exact) and the tolerance-mode kernels: pass-through on the fp16 roughness values around 0.05 and 0.75 under both
    approximate_with_ddgi settings, sky centres write 0, dead tiles copy; colour up to 6e4 in exact mode"""
    import torch
    from hybrid_rendering_amd import api_reflections
    from oracle import pyoracle_reflections as orf
    info = _info(w, h)
    gb = info["gb"]
    sob_d, sr_d = _tables()
    gb_d = helpers.to_cuda(gb)
    fi = hr.frame_inputs(gb_d, gb_d, _ubo(w, h), 0, 0, sob_d, sr_d, cur_full=gb_d)
    bnd, rows, resident = _band_args(info, band, tiling.HALO)
    for prm in (fc.REFLECTION_VARIANTS[:1] if band else fc.REFLECTION_VARIANTS):
        gp = api_reflections.RayTracedReflections(ctx, w, h, 0, band=bnd)
        gp.params.exact = exact
        for k, v in prm.items():
            setattr(gp.params, k, v)
        p = gp.params
        try:
            gp.temporal(fi)      # the trace image is the created pass's zeros: only the geometry records of this stage are used
            _put_tiles(gp, info["tiles"])
            for name in (("refl_in", "refl_hdr") if exact else ("refl_in",)):
                inp = info[name]
                for i in range(4):
                    src, dst = (gp.IMG_COLOR0 if i == 0 else gp.IMG_ATROUS0 + (i & 1)), gp.IMG_ATROUS0 + ((i & 1) ^ 1)
                    _put(gp.image(dst), np.full(inp.shape, SENTINEL, np.uint16))
                    _put(gp.image(src), inp)
                    gp.atrous_iteration(fi, i)
                    torch.cuda.synchronize()
                    got = helpers.bits16(gp.image(dst))
                    ref = _cached(("refl", name, w, h, tuple(sorted(prm.items())), i), lambda: orf.atrous(
                        inp, gb, info["tiles"], 1 << i, p.radius, p.phi_color, p.phi_normal, p.sigma_depth, p.approximate_with_ddgi))
                    what = f"reflections a-trous {name} {w}x{h} {prm} iteration {i}"
                    _check(got, ref, what, exact, lambda y, x: fc.describe(info, y, x, 1 << i, p.radius), rows, variance_channels=(3,), outlier_pixels=0)
                    if band:
                        _untouched(got.reshape(ref.shape), resident, what)
        finally:
            gp.close()


# ------------------------------------------------------------------------------------------------------------------------ route A: upsample
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("w,h", fc.UPSAMPLE_LOW)
def test_upsample(oracle, hr, ctx, w, h, exact):
    """csrc/upsample.h and denoise_fast_resolve.hip for the three passes at full sizes 2w, 2w + 1, 4w and 4w + 3 (the pass's low extent is
    full >> scale): 0 - 4 sky taps, opposite normals on all four taps (total weight 0 -> 0 / 1e-8), AO power 1.2 on results of 0, below 2^-10 and
    above 1, the clamp to edge at the first and last column and row"""
    import torch
    from hybrid_rendering_amd import api_reflections
    sob_d, sr_d = _tables()
    for scale, extra in fc.UPSAMPLE_FULL:
        u = _cached(("up", w, h, scale, extra), lambda: fc.craft_upsample(w, h, scale, extra))
        W, H = u["W"], u["H"]
        full_d, low_d = helpers.to_cuda(u["full"]), helpers.to_cuda(u["low"])
        fi = hr.frame_inputs(low_d, low_d, _ubo(W, H), 0, 0, sob_d, sr_d, cur_full=full_d, z_buffer_params=ZBP)
        passes = [("ao", hr.RayTracedAO(ctx, W, H, scale), "IMG_BLUR1", "IMG_UPSAMPLE", "ao_in", 1, 1.0, 1.2),
                  ("shadows", hr.RayTracedShadows(ctx, W, H, scale), "IMG_ATROUS0", "IMG_UPSAMPLE", "shadows_in", 1, 0.0, 0.0),
                  ("reflections", api_reflections.RayTracedReflections(ctx, W, H, scale), "IMG_ATROUS0", "IMG_UPSAMPLE", "refl_in", 4, 0.0, 0.0)]
        try:
            for name, gp, src, dst, key, ch, sky_value, power in passes:
                assert (gp.width, gp.height) == (w, h)
                gp.params.exact = exact
                low = u[key]
                _put(gp.image(getattr(gp, src)), low)
                gp.upsample(fi)
                torch.cuda.synchronize()
                got = helpers.bits16(gp.image(getattr(gp, dst)))
                ref = _cached(("up", name, w, h, scale, extra), lambda: oracle.upsample(
                    u["full"], u["low"], low if low.ndim == 3 else low[..., None], channels=ch, sky_value=sky_value, power=power))
                _check(got, ref, f"{name} upsample {W}x{H} over {w}x{h}", exact, lambda y, x: fc.describe_upsample(u, y, x))
        finally:
            for p in passes:
                p[1].close()


# ------------------------------------------------------------------------------------------------------------------------ route B
ROUTE_B_SHAPES = fc.SHAPES[1:]


def _route_b(w, h):
    info = _info(w, h)
    return info, _cached(("hist", w, h), lambda: fc.craft_history(info))


@pytest.mark.parametrize("prm", [dict(), dict(filter_iterations=2, feedback_iteration=0, power=2.0), dict(phi_normal=12.5)], ids=["default", "two_iterations", "phi12.5"])
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("w,h", ROUTE_B_SHAPES)
def test_shadows_denoise_through_the_temporal_stage(oracle, hr, ctx, w, h, exact, prm):
    """kf_shadows_atrous01 (iterations 0 + 1 in one launch, feedback copies out2 / out_first2) on a temporal output with fractional visibilities,
    non-zero variance and dead tiles whose variance is not 0"""
    import torch
    info, hist = _route_b(w, h)
    gb = info["gb"]
    gsc = hr.Scene(ctx, helpers.scene_data("cornell"))
    sob_d, sr_d = _tables()
    ubo = _ubo(w, h)
    gb_d = helpers.to_cuda(gb)
    fi = hr.frame_inputs(gb_d, gb_d, ubo, 0, 0, sob_d, sr_d)

    def run(gp):
        gp.params.exact = exact
        for k, v in prm.items():
            setattr(gp.params, k, v)
        gp.ray_trace(gsc, fi)
        _put(gp.image(gp.IMG_MASK), hist["shadow_mask"])
        _put(gp.image(gp.IMG_PREV), hist["shadows_hist"])
        _put(gp.image(gp.IMG_MOMENTS1), hist["moments"])       # ping_pong 0 reads moments[1]
        gp.denoise(fi)
        torch.cuda.synchronize()
        return dict(temporal=helpers.bits16(gp.image(gp.IMG_TEMPORAL)), moments=helpers.bits16(gp.image(gp.IMG_MOMENTS0)), tiles=gp.image(gp.IMG_TILES).cpu().numpy().copy(),
                    output=helpers.bits16(gp.output(hr.OUTPUT_ATROUS)), feedback=helpers.bits16(gp.image(gp.IMG_PREV)))

    fused = hr.RayTracedShadows(ctx, w, h)
    plain = _unfused(lambda: hr.RayTracedShadows(ctx, w, h))
    try:
        a = run(fused)
        p = fused.params
        n_it = p.filter_iterations
        tag = f"shadows {w}x{h} exact {exact} {prm}"
        if exact:
            tv, mom, tiles = _cached(("b_shadows_t", w, h), lambda: oracle.shadows_temporal(ubo, hist["shadow_mask"], gb, gb, hist["shadows_hist"], hist["moments"], p.alpha, p.moments_alpha))
            tell = lambda y, x: fc.describe(info, y, x)
            _check(a["temporal"], tv, f"{tag}: temporal output", 1, tell)
            _check(a["moments"], mom, f"{tag}: moments", 1, tell)
            assert np.array_equal(a["tiles"], tiles), f"{tag}: tile classes"
            img = tv
            for i in range(n_it):
                img = oracle.shadows_atrous(img, gb["gb2"], gb["gb3"], tiles, 1 << i, p.radius, p.phi_visibility, p.phi_normal, p.sigma_depth, p.power if i == n_it - 1 else 0.0)
                if i == p.feedback_iteration:
                    _check(a["feedback"], img, f"{tag}: feedback image (iteration {i})", 1, lambda y, x: fc.describe(info, y, x, 1 << i))
            _check(a["output"], img, f"{tag}: a-trous output", 1, lambda y, x: fc.describe(info, y, x, 1 << (n_it - 1)))
            return
        b = run(plain)
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{tag}: {k} of the fused launch differs from the unfused chain's in {int((a[k] != b[k]).sum())} values"
        assert np.array_equal(a["tiles"], fc.temporal_tiles(info)), f"{tag}: the temporal stage must reproduce the crafted tile pattern"
        src = b["temporal"].reshape(h, w, 2)
        for i in range(n_it):
            plain.atrous_iteration(fi, i)
            torch.cuda.synchronize()
            got = helpers.bits16(plain.image(plain.IMG_ATROUS0 if i & 1 else plain.IMG_ATROUS1)).reshape(src.shape)
            ref = oracle.shadows_atrous(src, gb["gb2"], gb["gb3"], b["tiles"], 1 << i, p.radius, p.phi_visibility, p.phi_normal, p.sigma_depth, p.power if i == n_it - 1 else 0.0)
            _check(got, ref, f"{tag}: iteration {i} against the oracle's iteration on the same image", 0, lambda y, x: fc.describe(info, y, x, 1 << i), variance_channels=(1,))
            if i == p.feedback_iteration:
                assert np.array_equal(got, a["feedback"].reshape(src.shape)), f"{tag}: the fused launch's feedback copy is iteration {i}'s image"
            src = got
        assert np.array_equal(src, a["output"].reshape(src.shape)), f"{tag}: the iterations one by one reproduce the fused chain's output"
    finally:
        fused.close(); plain.close(); gsc.close()


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("w,h", ROUTE_B_SHAPES)
def test_ao_denoise_through_the_temporal_stage(oracle, hr, ctx, w, h, exact):
    """kf_ao_blur_xy (X and Y in one launch, the X image in LDS) against the two launches, on a temporal output with dead tiles (AO 1 everywhere)"""
    import torch
    info, hist = _route_b(w, h)
    gb = info["gb"]
    gsc = hr.Scene(ctx, helpers.scene_data("cornell"))
    sob_d, sr_d = _tables()
    ubo, zb = _ubo(w, h), np.asarray(ZBP, np.float32)
    gb_d = helpers.to_cuda(gb)
    fi = hr.frame_inputs(gb_d, gb_d, ubo, 0, 0, sob_d, sr_d, z_buffer_params=ZBP)
    mh = (h + 3) // 4

    def run(gp):
        gp.params.exact = exact
        gp.ray_trace(gsc, fi)
        mask = gp.image(gp.IMG_MASK)
        _put(mask[:mh], hist["ao_mask"][0])
        _put(gp.image(gp.IMG_AO1), hist["ao_hist"])        # ping_pong 0 reads the [1] images
        _put(gp.image(gp.IMG_LEN1), hist["ao_len"])
        gp.denoise(fi)
        torch.cuda.synchronize()
        return dict(temporal=helpers.bits16(gp.image(gp.IMG_AO0)), length=helpers.bits16(gp.image(gp.IMG_LEN0)), tiles=gp.image(gp.IMG_TILES).cpu().numpy().copy(),
                    blur1=helpers.bits16(gp.image(gp.IMG_BLUR1)))

    fused = hr.RayTracedAO(ctx, w, h, 0)
    plain = _unfused(lambda: hr.RayTracedAO(ctx, w, h, 0))
    try:
        a = run(fused)
        p = fused.params
        tag = f"AO {w}x{h} exact {exact}"
        tx = lambda y, x: fc.describe(info, y, x, 1, p.blur_radius, direction=(1, 0))
        ty = lambda y, x: fc.describe(info, y, x, 1, p.blur_radius, direction=(0, 1))
        if exact:
            out, ln, tiles = _cached(("b_ao_t", w, h), lambda: oracle.ao_temporal(ubo, hist["ao_mask"], gb, gb, hist["ao_hist"], hist["ao_len"], p.alpha))
            _check(a["temporal"], out, f"{tag}: temporal AO", 1, tx)
            _check(a["length"], ln, f"{tag}: history length", 1, tx)
            assert np.array_equal(a["tiles"], tiles), f"{tag}: tile classes"
            b0 = oracle.ao_blur(out, gb["depth"], gb["gb2"], tiles, zb, (1, 0), p.blur_radius)
            _check(helpers.bits16(fused.image(fused.IMG_BLUR0)), b0, f"{tag}: blur X", 1, tx)
            _check(a["blur1"], oracle.ao_blur(b0, gb["depth"], gb["gb2"], tiles, zb, (0, 1), p.blur_radius), f"{tag}: blur Y", 1, ty)
            return
        b = run(plain)
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{tag}: {k} of the fused launch differs from the two launches' in {int((a[k] != b[k]).sum())} values"
        assert np.array_equal(a["tiles"], fc.temporal_tiles(info)), f"{tag}: the temporal stage must reproduce the crafted tile pattern"
        t_g = b["temporal"].reshape(h, w)
        x_g = helpers.bits16(plain.image(plain.IMG_BLUR0)).reshape(h, w)
        _check(x_g, oracle.ao_blur(t_g, gb["depth"], gb["gb2"], b["tiles"], zb, (1, 0), p.blur_radius), f"{tag}: blur X against the oracle's on the same image", 0, tx)
        _check(b["blur1"], oracle.ao_blur(x_g, gb["depth"], gb["gb2"], b["tiles"], zb, (0, 1), p.blur_radius), f"{tag}: blur Y against the oracle's on the same image", 0, ty)
    finally:
        fused.close(); plain.close(); gsc.close()


@pytest.mark.parametrize("prm", [dict(), dict(approximate_with_ddgi=0, blur_as_input=1, feedback_iteration=1), dict(blur_as_input=1, feedback_iteration=0, filter_iterations=2)],
                         ids=["default", "no_ddgi_feedback1", "two_iterations_feedback0"])
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("w,h", ROUTE_B_SHAPES)
def test_reflections_denoise_through_the_temporal_stage(oracle, hr, ctx, w, h, exact, prm):
    """kf_refl_atrous01 against the two launches; dead tiles are those whose roughness is below 0.05 everywhere (filter_cases.craft_history)"""
    import torch
    from hybrid_rendering_amd import api_reflections
    from oracle import pyoracle_reflections as orf
    info, hist = _route_b(w, h)
    gb = hist["gb_reflections"]
    sob_d, sr_d = _tables()
    ubo = _ubo(w, h)
    gb_d = helpers.to_cuda(gb)
    fi = hr.frame_inputs(gb_d, gb_d, ubo, 0, 0, sob_d, sr_d, cur_full=gb_d)

    def run(gp):
        gp.params.exact = exact
        for k, v in prm.items():
            setattr(gp.params, k, v)
        _put(gp.image(gp.IMG_TRACE), hist["trace"])
        _put(gp.image(gp.IMG_PREV if gp.params.blur_as_input else gp.IMG_COLOR1), hist["refl_hist"])
        _put(gp.image(gp.IMG_MOMENTS1), hist["refl_moments"])
        gp.denoise(fi)
        torch.cuda.synchronize()
        return dict(temporal=helpers.bits16(gp.image(gp.IMG_COLOR0)), moments=helpers.bits16(gp.image(gp.IMG_MOMENTS0)), tiles=gp.image(gp.IMG_TILES).cpu().numpy().copy(),
                    output=helpers.bits16(gp.output(hr.OUTPUT_ATROUS)), feedback=helpers.bits16(gp.image(gp.IMG_PREV)))

    fused = api_reflections.RayTracedReflections(ctx, w, h, 0)
    plain = _unfused(lambda: api_reflections.RayTracedReflections(ctx, w, h, 0))
    try:
        a = run(fused)
        p = fused.params
        n_it = p.filter_iterations
        tag = f"reflections {w}x{h} exact {exact} {prm}"
        if exact:
            oc, om, tiles = orf.temporal(ubo, hist["trace"], gb, gb, hist["refl_hist"], hist["refl_moments"], (0.0, 0.0, 0.0), p.alpha, p.moments_alpha, p.approximate_with_ddgi)
            tell = lambda y, x: fc.describe(info, y, x)
            _check(a["temporal"], oc, f"{tag}: temporal colour", 1, tell)
            _check(a["moments"], om, f"{tag}: moments", 1, tell)
            assert np.array_equal(a["tiles"], tiles), f"{tag}: tile classes"
            img = oc
            for i in range(n_it):
                img = orf.atrous(img, gb, tiles, 1 << i, p.radius, p.phi_color, p.phi_normal, p.sigma_depth, p.approximate_with_ddgi)
                if i == p.feedback_iteration and p.blur_as_input:
                    _check(a["feedback"], img, f"{tag}: feedback image (iteration {i})", 1, lambda y, x: fc.describe(info, y, x, 1 << i))
            _check(a["output"], img, f"{tag}: a-trous output", 1, lambda y, x: fc.describe(info, y, x, 1 << (n_it - 1)))
            return
        b = run(plain)
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{tag}: {k} of the fused launch differs from the unfused chain's in {int((a[k] != b[k]).sum())} values"
        assert np.array_equal(a["tiles"], fc.temporal_tiles(info)), f"{tag}: the temporal stage must reproduce the crafted tile pattern"
        src = b["temporal"].reshape(h, w, 4)
        for i in range(n_it):
            plain.atrous_iteration(fi, i)
            torch.cuda.synchronize()
            got = helpers.bits16(plain.image(plain.IMG_ATROUS0 if i & 1 else plain.IMG_ATROUS1)).reshape(src.shape)
            ref = orf.atrous(src, gb, b["tiles"], 1 << i, p.radius, p.phi_color, p.phi_normal, p.sigma_depth, p.approximate_with_ddgi)
            _check(got, ref, f"{tag}: iteration {i} against the oracle's iteration on the same image", 0, lambda y, x: fc.describe(info, y, x, 1 << i), variance_channels=(3,), outlier_pixels=0)
            if i == p.feedback_iteration and p.blur_as_input:
                assert np.array_equal(got, a["feedback"].reshape(src.shape)), f"{tag}: the fused launch's feedback copy is iteration {i}'s image"
            src = got
        assert np.array_equal(src, a["output"].reshape(src.shape)), f"{tag}: the iterations one by one reproduce the fused chain's output"
    finally:
        fused.close(); plain.close()
