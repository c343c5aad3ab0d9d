"""THE PIN at the HDR edge: the oracle against the reference's own shaders (oracle/refshim, as in tests/test_ref_shaders.py) on crafted
inputs that hold +inf, NaN, -0, 65504 and other values near the fp16 limit (tests/nonfinite_cases.py).  The reference's radiance has no upper
bound (an rgba16f store of anything >= 65520 is +inf), and the inf then runs through the probe update, the atlases, the probe-grid sample,
the reflections' denoiser, the deferred composite, TAA and the tone map.  Outputs are compared bit for bit except that two NaNs are equal
whatever their payload (helpers.assert_bits_equal_nan).  Every case also asserts that it is not vacuous: the reference's output holds the
edge values the case is about, next to finite texels."""
import numpy as np
import pytest

import helpers
import nonfinite_cases as nc
from hybrid_rendering_amd import synth, synth_env
from oracle import pyref

pytestmark = pytest.mark.skipif(not pyref.available(), reason="neither the reference tree nor a prebuilt oracle/_ref")


@pytest.fixture(scope="module")
def rh():
    from oracle import ref_harness
    return ref_harness


def _counts(bits):
    v = nc.f16(bits)
    return int(np.isnan(v).sum()), int(np.isinf(v).sum()), int(np.isfinite(v).sum())


def _frames(oracle, name, w, h, n=1, dolly=0.5, light_kind="default"):
    sd = helpers.scene_data(name)
    osc = oracle.Scene(sd)
    return sd, osc, helpers.make_frames(oracle, osc, name, w, h, n, dolly, light_kind)


@pytest.mark.parametrize("first_frame", [True, False])
def test_ddgi_probe_update_and_border_on_hdr_rays(oracle, rh, first_frame):
    """gi_irradiance_probe_update.comp / gi_depth_probe_update.comp + both border updates: +inf rays (a ray facing away from a texel is
    skipped, not weighted by 0: no inf * 0 = NaN), 65504 rays, a NaN ray, inf / NaN / miss distances (min(max_distance, NaN) is
    max_distance in the GLSL formula order), and inf / NaN texels of the previous atlases through the hysteresis"""
    from oracle import pyoracle_ddgi as od
    ddgi = nc.ddgi_grid()
    rad, dd = nc.probe_rays(ddgi)
    pirr, pdep = nc.prev_atlases(ddgi)
    ir = rh.ddgi_probe_update(ddgi, False, first_frame, rad, dd, pirr, pdep)
    dr = rh.ddgi_probe_update(ddgi, True, first_frame, rad, dd, pirr, pdep)
    io = od.probe_update(ddgi, False, first_frame, rad, dd, pirr)
    do = od.probe_update(ddgi, True, first_frame, rad, dd, pdep)
    helpers.assert_bits_equal_nan(io, ir, "irradiance probe update")
    helpers.assert_bits_equal_nan(do, dr, "depth probe update")
    helpers.assert_bits_equal_nan(od.border_update(ddgi, False, io), rh.ddgi_border_update(ddgi, False, ir.copy()), "irradiance border update")
    helpers.assert_bits_equal_nan(od.border_update(ddgi, True, do), rh.ddgi_border_update(ddgi, True, dr.copy()), "depth border update")
    # not vacuous: the +inf rays reach the irradiance (inf texels), the NaN ray poisons only the texels it faces, finite texels remain
    n_nan, n_inf, n_fin = _counts(ir[..., :3])
    assert n_inf > 0 and n_nan > 0 and n_fin > 10 * (n_inf + n_nan), (n_nan, n_inf, n_fin)
    side = int(ddgi["irradiance_probe_side_length"])
    p1 = nc.f16(ir[2:2 + side, 2 + (side + 2):2 + (side + 2) + side, :3])     # probe 1: two inf rays, no NaN ray
    assert np.isinf(p1).any() and np.isfinite(p1).any() and not np.isnan(p1).any()
    p2 = nc.f16(ir[2:2 + side, 2 + 2 * (side + 2):2 + 2 * (side + 2) + side, :3])  # probe 2: every ray at 65504 -> 0.95 * 65504, finite
    assert np.isfinite(p2).all() and (p2 > 6.0e4).mean() > 0.5 if first_frame else np.isfinite(p2).all()
    dv = nc.f16(dr)
    interior = np.zeros(dv.shape[:2], bool)
    sd_ = int(ddgi["depth_probe_side_length"])
    for gy in range(int(ddgi["probe_counts"][2])):
        for gx in range(int(ddgi["probe_counts"][0] * ddgi["probe_counts"][1])):
            interior[gy * (sd_ + 2) + 2:gy * (sd_ + 2) + 2 + sd_, gx * (sd_ + 2) + 2:gx * (sd_ + 2) + 2 + sd_] = True
    if first_frame:
        assert np.isfinite(dv).all(), "a NaN / inf ray distance must not reach the depth moments"
    else:
        assert np.isinf(dv[interior]).any() and np.isnan(dv[interior]).any() and np.isfinite(dv[interior]).mean() > 0.99


@pytest.mark.parametrize("name", ["cornell", "sponza_small"])
def test_ddgi_sample_probe_grid_on_poisoned_atlases(oracle, rh, name):
    """gi_sample_probe_grid.comp on atlases with inf / NaN irradiance texels, overflowed depth moments (inf - inf) and a whole +inf probe"""
    from oracle import pyoracle_ddgi as od
    w, h = 64, 48
    sd, osc, frames = _frames(oracle, name, w, h, 2, 1.0)
    lo, hi = sd.bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 2, 3), rays_per_probe=32, normal_bias=1.0 if name == "cornell" else 0.1)
    op = od.DDGIPass(ddgi)
    rng = np.random.RandomState(11)
    sky = synth_env.sky_cubemap(8)
    for f in range(2):
        op.render(osc, frames[f]["ubo"], frames[f]["gb"], sky, synth_env.random_orientation(rng), f)
    irr, dep = nc.poison_atlases(ddgi, *op.current_read())
    fr = frames[-1]
    for gi_intensity in (1.0, 0.0):
        ref = rh.ddgi_sample_probe_grid(fr["ubo"], ddgi, fr["gb"], gi_intensity, irr, dep)
        got = od.sample_probe_grid(fr["ubo"], ddgi, fr["gb"]["depth"], fr["gb"]["gb2"], gi_intensity, irr, dep)
        helpers.assert_bits_equal_nan(got, ref, f"{name}: sampled irradiance, gi_intensity {gi_intensity}")
    n_nan, n_inf, n_fin = _counts(ref[..., :3])
    assert n_nan + n_inf > 0 and n_fin > 0, (n_nan, n_inf, n_fin)


@pytest.mark.parametrize("approx", [True, False])
def test_reflections_denoiser_on_nan_and_signed_zero(oracle, rh, approx):
    """reflections_denoise_reprojection.comp and reflections_denoise_atrous.comp x3 with NaN, +inf and 65504 texels (and -0 ones) in the
    traced colour and in the colour / moments history"""
    from oracle import pyoracle_reflections as orf
    W, H = 64, 48
    sd, osc, frames = _frames(oracle, "sponza_small", W, H, 2, 0.5)
    cur, prev = frames[1]["gb"], frames[0]["gb"]
    inp = nc.hdr_colour(H, W, seed=5)
    hist = nc.hdr_colour(H, W, seed=6)
    hm = nc.hdr_colour(H, W, seed=7)
    p = orf.ReflectionsPass(W, H).p
    cd = (-1.0, 0.0, 0.0)
    oc, om, den, cpy = rh.reflections_temporal(frames[1]["ubo"], inp, cur, prev, hist, hm, cd, p["alpha"], p["moments_alpha"], approx)
    gc, gm, tiles = orf.temporal(frames[1]["ubo"], inp, cur, prev, hist, hm, cd, p["alpha"], p["moments_alpha"], approx)
    helpers.assert_bits_equal_nan(gc, oc, "reprojected colour")
    helpers.assert_bits_equal_nan(gm, om, "moments")
    rt = np.zeros_like(tiles)
    rt[den[:, 1] // 8, den[:, 0] // 8] = 1
    assert np.array_equal(rt, tiles)
    n_nan, n_inf, n_fin = _counts(oc)
    assert n_nan > 0 and n_inf > 0 and n_fin > 0.9 * oc.size, (n_nan, n_inf, n_fin)
    # the -0 input texels do not reach these outputs (no stage output holds -0: the blends with the +0-based history give +0), so the case
    # pins NaN and inf only; signed zero is pinned by tests/test_helpers_bits.py and the GLSL-order min / max sites
    img = oc
    for i in range(3):
        ref = rh.reflections_atrous(img, cur, den, cpy, 1 << i, p["radius"], p["phi_color"], p["phi_normal"], p["sigma_depth"], approx)
        got = orf.atrous(img, cur, tiles, 1 << i, p["radius"], p["phi_color"], p["phi_normal"], p["sigma_depth"], approx)
        helpers.assert_bits_equal_nan(got, ref, f"a-trous iteration {i}")
        img = ref
    n_nan, n_inf, n_fin = _counts(img)
    assert n_nan > 0 and n_fin > 0, (n_nan, n_inf, n_fin)


@pytest.mark.parametrize("approx", [1, 0])
def test_reflections_trace_on_poisoned_atlases(oracle, rh, approx):
    """reflections_ray_trace.rgen + .rchit on metallic = 1 materials (kD = 0) with a +inf irradiance probe: the hit's indirect term is
    0 * inf = NaN, and the stored min(color, vec3(0.7)) keeps the NaN in the GLSL formula order (the reversed comparison stored 0.7)"""
    from oracle import pyoracle_reflections as orf
    W, H = 48, 32
    sd = nc.metallic_scene(helpers.scene_data("sponza_small"))
    osc = oracle.Scene(sd)
    frames = helpers.make_frames(oracle, osc, "sponza_small", W, H, 1, 1.0)
    rsc = rh.RefScene(sd)
    lo, hi = sd.bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 2, 3), rays_per_probe=32, normal_bias=0.1)
    sky = synth_env.sky_cubemap(8)
    env = dict(sky=sky, prefiltered=synth_env.prefiltered_chain(sky, 4), pre_size=8, pre_levels=4, lut=synth_env.brdf_lut(8))
    irr, dep = nc.inf_atlases(ddgi)
    sob, sr = synth.blue_noise_tables()
    cur = frames[0]["gb"]
    tp = orf.TraceParams(0.5, 0.8, 0, 1, approx, 0.5, 0.5, 0.05)
    a, rays = orf.ray_trace(osc, frames[0]["ubo"], ddgi, cur, sob, sr, tp, env, irr, dep)
    b = rh.reflections_ray_trace(osc, rsc, frames[0]["ubo"], ddgi, cur, sob, sr, tp, env, irr, dep)
    helpers.assert_bits_equal_nan(a, b, "reflections trace image")
    n_nan, n_inf, n_fin = _counts(b[..., :3])
    assert n_nan > 0 and n_fin > 0, (n_nan, n_inf, n_fin)


def test_taa_tone_map_and_deferred_on_hdr_inputs(oracle, rh):
    """taa.comp (history and current colour with inf, 65504, >= 1e4, NaN), tone_map.frag on the result and on the raw HDR image, and
    deferred.frag with a NaN / inf / huge GI image and reflections image"""
    from oracle import pyoracle_deferred as odf, pyoracle_post as opost
    W, H = 48, 32
    sd, osc, frames = _frames(oracle, "sponza_small", W, H, 2, 0.5)
    col0, col1 = nc.hdr_colour(H, W, seed=8), nc.hdr_colour(H, W, seed=9)
    t = opost.TAAPass(W, H)
    for k, col in enumerate((col0, col1)):
        t.reset = (k == 0)
        t.update(k)
        t.render(col, frames[k]["gb"], k & 1)
        ref = rh.taa_resolve(col, t.images[int(not (k & 1))], frames[k]["gb"], t.jitter, t.feedback_min, t.feedback_max, t.sharpen)
        helpers.assert_bits_equal_nan(t.output(k & 1), ref, f"TAA frame {k}")
    # taa.comp resolves in a tone-mapped space and stores clamp(.., 0, 1): the inf / huge texels saturate at 1, the NaN ones stay NaN
    n_nan, n_inf, n_fin = _counts(ref)
    assert n_nan > 0 and n_fin > 0 and (nc.f16(ref) == 1.0).any(), (n_nan, n_inf, n_fin)
    for img in (ref, col1):
        for single, exposure in ((False, 1.0), (True, 1.0), (False, 0.37)):
            a, b = opost.tone_map(img, single, exposure), rh.tone_map(img, single, exposure)
            helpers.assert_bits_equal_nan(a.view(np.uint32), b.view(np.uint32), f"tone map single={single} exposure={exposure}")
    # not vacuous: the NaN and inf texels leave the [0, 1] range of the ACES curve (clamp keeps the NaN, then pow of the NaN), 65504 saturates
    t1 = rh.tone_map(col1, False, 1.0)
    assert ((t1[..., :3] > 1.0) | np.isnan(t1[..., :3])).any() and (t1[..., :3] == 1.0).any() and (t1[..., :3] < 1.0).mean() > 0.9
    assert np.isnan(rh.tone_map(col1, True, 1.0)).any()
    sky = synth_env.sky_cubemap(16)
    env = dict(sky=sky, prefiltered=synth_env.prefiltered_chain(sky, 5), pre_size=16, pre_levels=5, lut=synth_env.brdf_lut(16))
    sh9 = synth_env.sh9_from_cubemap(sky)
    rng = np.random.RandomState(3)
    shadow, ao = nc.h16(rng.uniform(0, 1, (H, W))), nc.h16(rng.uniform(0, 1, (H, W)))
    gi, refl = nc.hdr_colour(H, W, seed=10), nc.hdr_colour(H, W, seed=12)
    for kind in ("default", "point"):
        sdk, osck, fk = _frames(oracle, "sponza_small", W, H, 1, 0.0, kind)
        for flags in (15, 8, 4):
            a = odf.shade(fk[0]["ubo"], fk[0]["gb"], shadow, ao, refl, gi, flags, sh9, env, skybox=False)
            b = rh.deferred_shade(fk[0]["ubo"], fk[0]["gb"], shadow, ao, refl, gi, flags, sh9, env)
            helpers.assert_bits_equal_nan(a, b, f"deferred {kind} flags {flags}")
            n_nan, n_inf, n_fin = _counts(b[..., :3])
            assert n_nan + n_inf > 0 and n_fin > 0, (kind, flags, n_nan, n_inf, n_fin)
