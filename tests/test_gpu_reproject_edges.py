"""The three temporal kernels on the adversarial G-buffers of tests/reproject_cases.py (families A-G: shifts across the borders, tap subsets and
the 3x3 fallback, sumw at 0.01, plane distance at 5, cos^2 at 0.1, sky; mirrors with a curvature checkerboard for the reflections), against the oracle.

exact = 1: every stage image of every frame bit for bit.  exact = 0: the rule of docs/TOLERANCE.md with the arguments tests/test_gpu_tolerance.py
passes for the same image, and — families D and E — the set of pixels whose reprojection was rejected must be the oracle's.  The temporal stages
store min(32, success ? length + 1 : 1) (reproject_cases.reset_set): a rejected ladder pixel stores 1, an accepted one >= 2.  Every tolerance sequence
runs twice: with the G-buffer tensors kept alive so that frame f's `prev` tensors ARE frame f - 1's `cur` tensors (the pass reads its own geometry
records; HR_DEBUG_REQUIRE_GEO, set while that pass is created, makes its temporal stage fail from the second frame on if it does
not), and with `prev` cloned to other addresses (it reads the caller's images); both against the oracle, and equal to each other."""
import contextlib
import os

import numpy as np
import pytest

import helpers
import reproject_cases as rc
from hybrid_rendering_amd import synth, synth_env
from test_gpu_tolerance import (ATROUS_OUTLIERS, DDGI_OUTLIERS, INTERMEDIATE_FLOOR, REFL_OUTLIERS, compare16, compare_trace, tiles_close, upsample_scale)

pytestmark = pytest.mark.gpu

CASES = [(n, w, h) for n in rc.SCENES for (w, h) in rc.SIZES]
_ref = {}


def _tables():
    import torch
    sob, sr = synth.blue_noise_tables()
    return sob, sr, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()


def _oracle_run(oracle, what, name, w, h):
    """the oracle's stage images of all six frames, computed once per (pass, scene, size) and shared by the exact and the tolerance test"""
    key = (what, name, w, h)
    if key in _ref:
        return _ref[key]
    osc, frames, info = rc.sequence(oracle, name, w, h)
    sob, sr = synth.blue_noise_tables()
    out = []
    if what == "shadows":
        op = oracle.ShadowsPass(w, h)
        for f, fr in enumerate(frames):
            op.render(osc, fr["ubo"], fr["gb"], frames[f - 1 if f else 0]["gb"], sob, sr, f)
            out.append(dict(op.stages, feedback=op.prev_image.copy()))
    elif what == "ao":
        op = oracle.AOPass(w, h, spp=2, zbp=synth.z_buffer_params())
        for f, fr in enumerate(frames):
            op.render(osc, fr["ubo"], fr["gb"], frames[f - 1 if f else 0]["gb"], sob, sr, f)
            out.append(dict(op.stages))
    else:
        from oracle import pyoracle_ddgi as od, pyoracle_reflections as orf
        ddgi, sky, env_np = _gi_setup(name)
        dp, op = od.DDGIPass(ddgi), orf.ReflectionsPass(w, h)
        gbr = _reflection_frames(frames)
        rng = np.random.RandomState(7)
        for f, fr in enumerate(frames):
            orient = synth_env.random_orientation(rng)
            dp.render(osc, fr["ubo"], gbr[f], sky, orient, f)
            irr, dep = dp.current_read()
            op.render(osc, fr["ubo"], ddgi, gbr[f], gbr[f - 1 if f else 0], sob, sr, f, env_np, irr, dep, camera_delta=_delta(f), ping_pong=bool(f & 1))
            out.append(dict(op.stages, irr=irr.copy(), dep=dep.copy(), ddgi_output=dp.stages["output"].copy(), orient=orient))
    _ref[key] = out
    return out


def _delta(f):
    return (0.0, 0.0, 0.0) if f == 0 else (-1.0, 0.0, 0.0)


def _gi_setup(name):
    lo, hi = helpers.scene_data(name).bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 3, 3), rays_per_probe=32, normal_bias=1.0 if name == "cornell" else 0.1)
    sky = synth_env.sky_cubemap(16)
    return ddgi, sky, dict(sky=sky, prefiltered=synth_env.prefiltered_chain(sky, 5), pre_size=16, pre_levels=5, lut=synth_env.brdf_lut(16))


def _reflection_frames(frames):
    """family G: every surface pixel a mirror in all six frames, the curvature checkerboard on frames H and C"""
    key = id(frames)
    if ("gbr", key) not in _ref:
        _ref[("gbr", key)] = [rc.reflections_variant(fr["gb"], checker=f in (rc.FRAME_H, rc.FRAME_C)) for f, fr in enumerate(frames)]
    return _ref[("gbr", key)]


def _inputs(gbs, records):
    """per frame (cur, prev) device G-buffers.  records: prev IS the preceding cur (same tensors, kept alive); else a clone at other addresses"""
    cur = [helpers.to_cuda(g) for g in gbs]
    prev = [cur[f - 1 if f else 0] if records else {k: v.clone() for k, v in cur[f - 1 if f else 0].items()} for f in range(len(cur))]
    return cur, prev


@contextlib.contextmanager
def _creating(exact, records):
    """Around the creation of a pass (its switches are read there).  The tolerance run on the records path sets HR_DEBUG_REQUIRE_GEO: from the
    second frame on the temporal stage then FAILS if it does not reproject from the pass's own records (the choice is otherwise silent, from pointer
    equality), so that this run cannot pass on the caller's images.  The other runs are created without it."""
    old = os.environ.pop("HR_DEBUG_REQUIRE_GEO", None)
    if records and not exact:
        os.environ["HR_DEBUG_REQUIRE_GEO"] = "1"
    try:
        yield
    finally:
        os.environ.pop("HR_DEBUG_REQUIRE_GEO", None)
        if old is not None:
            os.environ["HR_DEBUG_REQUIRE_GEO"] = old


def _equal(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    got = got.reshape(ref.shape)
    assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.size} values differ from the oracle's; first at {np.argwhere(got != ref)[:4].tolist()}"


def _verdicts(info, got_len, ref_len, what):
    """families D and E: the rejected set of the stored history length must be the oracle's; names the tap if not"""
    g, r = rc.reset_set(np.asarray(got_len).reshape(np.asarray(ref_len).shape)), rc.reset_set(ref_len)
    sel = (info["family"] == rc.FAMILY["D"]) | (info["family"] == rc.FAMILY["E"])
    bad = np.argwhere((g != r) & sel)
    msg = "; ".join(f"{rc.describe(info, int(y), int(x))}: oracle {'rejects' if r[y, x] else 'accepts'}, GPU {'rejects' if g[y, x] else 'accepts'}" for y, x in bad[:8])
    assert not len(bad), f"{what}: {len(bad)} flipped history-tap verdicts on the D / E stripes: {msg}"


# ------------------------------------------------------------------------------------------------------------------------ shadows
def _run_shadows(oracle, hr, ctx, name, w, h, exact, records):
    import torch
    osc, frames, info = rc.sequence(oracle, name, w, h)
    ref = _oracle_run(oracle, "shadows", name, w, h)
    gsc = hr.Scene(ctx, helpers.scene_data(name))
    sob, sr, sob_d, sr_d = _tables()
    with _creating(exact, records):
        gp = hr.RayTracedShadows(ctx, w, h)
    gp.params.exact = exact
    cur, prev = _inputs([fr["gb"] for fr in frames], records)
    images = []
    for f, fr in enumerate(frames):
        gp.render(gsc, hr.frame_inputs(cur[f], prev[f], fr["ubo"], f, f & 1, sob_d, sr_d))
        torch.cuda.synchronize()
        st, tag = ref[f], f"shadows {name} {w}x{h} exact {exact} frame {f}"
        img = dict(mask=gp.image(gp.IMG_MASK).cpu().numpy().view(np.uint32), tiles=gp.image(gp.IMG_TILES).cpu().numpy(), temporal=helpers.bits16(gp.image(gp.IMG_TEMPORAL)),
                   moments=helpers.bits16(gp.image(gp.IMG_MOMENTS1 if f & 1 else gp.IMG_MOMENTS0)), output=helpers.bits16(gp.output(hr.OUTPUT_ATROUS)),
                   feedback=helpers.bits16(gp.image(gp.IMG_PREV)))
        images.append(img)
        _equal(img["mask"], st["mask"], f"{tag}: mask")
        assert gp.ray_count() == st["rays"]
        if exact:
            for k in ("tiles", "temporal", "moments", "output", "feedback"):
                _equal(img[k], st[k], f"{tag}: {k}")
            continue
        if f == rc.FRAME_C:
            _verdicts(info, img["moments"].reshape(st["moments"].shape)[..., 2], st["moments"][..., 2], tag)
        ex = tiles_close(img["tiles"].reshape(st["tiles"].shape), st["tiles"], tag, shape=(h, w))
        compare16(img["temporal"].reshape(st["temporal"].shape), st["temporal"], f"{tag} temporal", abs_floor=INTERMEDIATE_FLOOR)
        compare16(img["moments"].reshape(st["moments"].shape), st["moments"], f"{tag} moments (m1, m2, history length, 0)", abs_floor=INTERMEDIATE_FLOOR)
        compare16(img["output"].reshape(st["output"].shape), st["output"], f"{tag} denoised visibility + filtered variance", exclude=ex, variance_channels=(1,), outlier_pixels=ATROUS_OUTLIERS)
        compare16(img["feedback"].reshape(st["feedback"].shape), st["feedback"], f"{tag} feedback image", exclude=ex, variance_channels=(1,), outlier_pixels=ATROUS_OUTLIERS)
    gp.close(); gsc.close()
    return images


# ------------------------------------------------------------------------------------------------------------------------ AO
def _run_ao(oracle, hr, ctx, name, w, h, exact, records):
    import torch
    osc, frames, info = rc.sequence(oracle, name, w, h)
    ref = _oracle_run(oracle, "ao", name, w, h)
    gsc = hr.Scene(ctx, helpers.scene_data(name))
    sob, sr, sob_d, sr_d = _tables()
    zbp = synth.z_buffer_params()
    with _creating(exact, records):
        gp = hr.RayTracedAO(ctx, w, h, 0)
    gp.params.spp, gp.params.exact = 2, exact
    cur, prev = _inputs([fr["gb"] for fr in frames], records)
    images, mh = [], (h + 3) // 4
    for f, fr in enumerate(frames):
        gp.render(gsc, hr.frame_inputs(cur[f], prev[f], fr["ubo"], f, f & 1, sob_d, sr_d, z_buffer_params=zbp))
        torch.cuda.synchronize()
        st, tag = ref[f], f"AO {name} {w}x{h} exact {exact} frame {f}"
        img = dict(mask=gp.image(gp.IMG_MASK).cpu().numpy().view(np.uint32)[:2 * mh].reshape(2, mh, -1), tiles=gp.image(gp.IMG_TILES).cpu().numpy(),
                   temporal=helpers.bits16(gp.image(gp.IMG_AO1 if f & 1 else gp.IMG_AO0)), length=helpers.bits16(gp.image(gp.IMG_LEN1 if f & 1 else gp.IMG_LEN0)),
                   blur1=helpers.bits16(gp.image(gp.IMG_BLUR1)), output=helpers.bits16(gp.output(hr.OUTPUT_UPSAMPLE)))
        images.append(img)
        _equal(img["mask"], st["mask"], f"{tag}: masks")
        assert gp.ray_count() == st["rays"]
        if exact:
            for k in ("tiles", "temporal", "length", "blur1", "output"):
                _equal(img[k], st[k], f"{tag}: {k}")
            continue
        if f == rc.FRAME_C:
            _verdicts(info, img["length"], st["length"], tag)
        ex = tiles_close(img["tiles"].reshape(st["tiles"].shape), st["tiles"], tag, shape=(h, w))
        compare16(img["temporal"].reshape(st["temporal"].shape), st["temporal"], f"{tag} temporal AO")
        compare16(img["blur1"].reshape(st["blur1"].shape), st["blur1"], f"{tag} blurred AO", exclude=ex)
        compare16(img["output"].reshape(st["output"].shape), st["output"], f"{tag} AO output", exclude=ex)
    gp.close(); gsc.close()
    return images


# ------------------------------------------------------------------------------------------------------------------------ reflections
def _run_reflections(oracle, hr, ctx, name, w, h, exact, records):
    import torch
    from hybrid_rendering_amd import api_gi, api_reflections
    osc, frames, info = rc.sequence(oracle, name, w, h)
    ref = _oracle_run(oracle, "reflections", name, w, h)
    gsc = hr.Scene(ctx, helpers.scene_data(name))
    sob, sr, sob_d, sr_d = _tables()
    ddgi, sky, env_np = _gi_setup(name)
    f16 = lambda a: torch.from_numpy(a).cuda().view(torch.float16)
    env = api_gi.environment(f16(sky), f16(env_np["prefiltered"]), 16, 5, f16(env_np["lut"]))
    g_ddgi = api_gi.DDGI(ctx, w, h, ddgi)
    with _creating(exact, records):
        gp = api_reflections.RayTracedReflections(ctx, w, h, 0)
    g_ddgi.params.exact = gp.params.exact = exact
    cur, prev = _inputs(_reflection_frames(frames), records)
    images = []
    for f, fr in enumerate(frames):
        st, tag = ref[f], f"reflections {name} {w}x{h} exact {exact} frame {f}"
        g_ddgi.render(gsc, hr.frame_inputs(cur[f], None, fr["ubo"], f, f & 1, sob_d, sr_d), env, st["orient"])
        gp.set_camera_delta(_delta(f))
        gp.render(gsc, hr.frame_inputs(cur[f], prev[f], fr["ubo"], f, f & 1, sob_d, sr_d, cur_full=cur[f]), env, g_ddgi)
        torch.cuda.synchronize()
        gi, gd = g_ddgi.current_read()
        _equal(helpers.bits16(gi), st["irr"], f"{tag}: DDGI irradiance atlas")
        _equal(helpers.bits16(gd), st["dep"], f"{tag}: DDGI depth atlas")
        img = dict(trace=helpers.bits16(gp.image(gp.IMG_TRACE)), tiles=gp.image(gp.IMG_TILES).cpu().numpy(), temporal=helpers.bits16(gp.image(gp.IMG_COLOR1 if f & 1 else gp.IMG_COLOR0)),
                   moments=helpers.bits16(gp.image(gp.IMG_MOMENTS1 if f & 1 else gp.IMG_MOMENTS0)), atrous=helpers.bits16(gp.output(hr.OUTPUT_ATROUS)),
                   output=helpers.bits16(gp.output(hr.OUTPUT_UPSAMPLE)), ddgi_output=helpers.bits16(g_ddgi.output()))
        images.append(img)
        assert gp.ray_count() == st["rays"]
        shp = st["temporal"].shape
        if exact:
            _equal(img["ddgi_output"], st["ddgi_output"], f"{tag}: DDGI probe-grid sample")
            for k in ("trace", "tiles", "temporal", "moments"):
                _equal(img[k], st[k], f"{tag}: {k}")
            _equal(img["atrous"], st["atrous"][-1], f"{tag}: a-trous output")
            _equal(img["output"], st["output"], f"{tag}: output")
            continue
        compare16(img["ddgi_output"].reshape(st["ddgi_output"].shape), st["ddgi_output"], f"{tag} DDGI probe-grid sample", outlier_pixels=DDGI_OUTLIERS)
        compare_trace(img["trace"].reshape(st["trace"].shape), st["trace"], f"{tag} reflection trace image")
        if f == rc.FRAME_C:
            _verdicts(info, img["moments"].reshape(shp)[..., 2], st["moments"][..., 2], tag)
        ex = tiles_close(img["tiles"].reshape(st["tiles"].shape), st["tiles"], tag, shape=(h, w))
        compare16(img["temporal"].reshape(shp), st["temporal"], f"{tag} temporal colour + variance", variance_channels=(3,), outlier_pixels=REFL_OUTLIERS)
        compare16(img["moments"].reshape(shp), st["moments"], f"{tag} moments (m1, m2, history length, 0)", outlier_pixels=REFL_OUTLIERS)
        compare16(img["atrous"].reshape(shp), st["atrous"][-1], f"{tag} a-trous colour + variance", exclude=ex, variance_channels=(3,), outlier_pixels=REFL_OUTLIERS)
        compare16(img["output"].reshape(st["output"].shape), st["output"], f"{tag} reflections output", exclude=ex, variance_channels=(3,), outlier_scale=upsample_scale(0), outlier_pixels=REFL_OUTLIERS)
    gp.close(); g_ddgi.close(); gsc.close()
    return images


RUNNERS = dict(shadows=_run_shadows, ao=_run_ao, reflections=_run_reflections)


@pytest.mark.parametrize("name,w,h", CASES)
@pytest.mark.parametrize("what", list(RUNNERS))
def test_parity_mode_is_bit_exact(oracle, hr, ctx, what, name, w, h):
    RUNNERS[what](oracle, hr, ctx, name, w, h, 1, True)


@pytest.mark.parametrize("name,w,h", CASES)
@pytest.mark.parametrize("what", list(RUNNERS))
def test_tolerance_mode_on_both_history_paths(oracle, hr, ctx, what, name, w, h):
    if os.environ.get("HR_GEO_HISTORY") == "0":
        pytest.skip("HR_GEO_HISTORY=0 (developer A/B switch): no record path to test")
    a = RUNNERS[what](oracle, hr, ctx, name, w, h, 0, True)      # the pass's own geometry records
    b = RUNNERS[what](oracle, hr, ctx, name, w, h, 0, False)     # the caller's previous G-buffer
    for f, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert np.array_equal(x[k], y[k]), f"{what} {name} {w}x{h} frame {f}: {k} from the records differs from {k} from the caller's images in {int((x[k] != y[k]).sum())} values"
