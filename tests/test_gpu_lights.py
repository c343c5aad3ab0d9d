"""Extra lights on the GPU (include/hr_lights.h): the LIGHTS instantiations of k_ddgi_trace, k_refl_trace and k_ground_truth and the primary-surface
pass hr_lights, through identities that need no new reference.  The SWAP IDENTITY carries the weight: a scene whose UBO light has intensity 0 and
whose list is [L] must give the bits of the present code under UBO light L with an empty list, and the present code is pinned to the reference's
shaders by the existing suite.  On a flat, a private-copy and a shared scene over the same world-space triangles (tests/lights_cases.py), with
cutouts on for flat and shared."""
import numpy as np
import pytest

import helpers
import lights_cases as lc
from hybrid_rendering_amd import synth, synth_env
from test_gpu_emission import make as make_kind, rig_for, ulp16_at_larger
from test_gpu_shared_passes import Passes, assert_equal_snapshots, gbuffer_np

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = [("flat", False), ("private", False), ("shared", False), ("flat", True), ("shared", True)]
IMAGES = ("ddgi_radiance", "ddgi_direction_distance", "ddgi_irradiance", "ddgi_depth", "refl_trace", "refl_atrous", "ground_truth", "ground_truth_indirect")


def make(hr, ctx, kind, cutout, isd=None):
    isd = lc.world() if isd is None else isd
    s = make_kind(hr, ctx, lc.hidden_cubes(isd) if cutout else isd, kind)
    return s.set_alpha_cutoffs(lc.cutoffs()) if cutout else s


def all_mirrors(cur):
    cur["gb3"][..., 0][cur["depth"] != 1.0] = np.float16(0.03).view(np.uint16)
    return cur


def run_frames(hr, ctx, scenes, frames=2, infinite_bounces=1, W=lc.W, H=lc.H, before_frame=None):
    """`frames` frames with temporal feedback of AO, DDGI, reflections and the ground truth (trace_indirect 0, and 1 with max_ray_bounces 3) over
    every scene: tag -> (scene, its UBO light).  All from the first scene's G-buffer.  Per frame: tag -> snapshot"""
    import torch
    from hybrid_rendering_amd import api_post
    rig = rig_for(W, H)
    sets = {tag: Passes(hr, ctx, rig, 1) for tag in scenes}
    gt1 = {tag: api_post.GroundTruthPathTracer(ctx, W, H) for tag in scenes}
    for p in gt1.values():
        p.params.trace_indirect, p.params.max_ray_bounces = 1, 3
    for p in sets.values():
        p.gi.params.infinite_bounces = infinite_bounces
    rng = np.random.RandomState(4)
    first = next(iter(scenes.values()))[0]
    out, prev = [], None
    for f in range(frames):
        if before_frame:
            before_frame(f)
        orient = synth_env.random_orientation(rng)
        snap = {}
        cur = None
        for tag, (scene, light) in scenes.items():
            ubo = synth.make_ubo(lc.camera(W / H), None, light)
            if cur is None:
                cur = all_mirrors(gbuffer_np(first, ubo, W, H))      # the G-buffer does not depend on the light
                prev = prev if prev is not None else cur
            fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
            snap[tag] = sets[tag].render(scene, fi, ubo, orient)
            gt1[tag].render(scene, ubo, rig.env)
            torch.cuda.synchronize()
            snap[tag]["ground_truth_indirect"] = helpers.bits16(gt1[tag].output())
            snap[tag]["gt_rays"] = sets[tag].gt.ray_count()
        out.append(snap)
        prev = cur
    for p in list(sets.values()) + list(gt1.values()):
        p.close()
    return out


def lit_share(bits):
    return float((bits[..., :3] != 0).any(-1).mean())


@pytest.mark.parametrize("kind,cutout", KINDS)
@pytest.mark.parametrize("which", list(lc.LIGHTS))
def test_swap_identity_in_the_hit_shaders(hr, ctx, kind, cutout, which):
    """item 1: scene A under UBO light L with no list against scene B under the same light at intensity 0 with list [L] — DDGI radiance,
    direction / distance and both atlases with infinite bounces on and off, the reflections trace image and its a-trous output, the ground truth with
    trace_indirect 0 and 1 (max_ray_bounces 3), two frames with feedback: equal bit for bit.  The ray counts differ (B traces the dark UBO light's
    ray too) and are not compared."""
    L = lc.LIGHTS[which]()
    for bounces in (1, 0):
        a, b = make(hr, ctx, kind, cutout), make(hr, ctx, kind, cutout).set_lights(lc.records(L))
        assert b.get_lights().tobytes() == lc.records(L).tobytes() and a.get_lights().shape == (0, 4, 4)
        frames = run_frames(hr, ctx, dict(a=(a, L), b=(b, lc.dark(L))), 2, bounces)
        for f, snap in enumerate(frames):
            assert_equal_snapshots(snap["b"], snap["a"], f"{kind} cutout={cutout} {which}, infinite bounces {bounces}, frame {f}: list [L] against UBO light L", keys=IMAGES)
            assert snap["b"]["refl_rays"] > snap["a"]["refl_rays"] and snap["b"]["gt_rays"] > snap["a"]["gt_rays"], "each traced list ray is counted"
            for k in ("ddgi_radiance", "refl_trace", "ground_truth", "ground_truth_indirect"):
                assert lit_share(snap["a"][k]) > 0.3, f"{which}: {k} is lit on {lit_share(snap['a'][k]):.2f} of its texels: equality would mean little"
        # and the light matters: under the dark UBO light without a list the images are others
        a.close(); b.close()
    c = make(hr, ctx, kind, cutout)
    dark = run_frames(hr, ctx, dict(c=(c, lc.dark(L))), 1, 0)[0]["c"]
    assert not np.array_equal(dark["ddgi_radiance"], frames[0]["a"]["ddgi_radiance"]) and not np.array_equal(dark["refl_trace"], frames[0]["a"]["refl_trace"])
    c.close()


# ---- the primary pass -------------------------------------------------------------------------------------------------------------------------------
def primary_setup(hr, ctx, scene, W, H, cam, light):
    """(rig with a black environment, frame inputs, numpy G-buffer, ubo) of `scene` seen by `cam` under UBO light `light`"""
    rig = rig_for(W, H, black_sky=True)
    ubo = synth.make_ubo(cam, None, light)
    cur = gbuffer_np(scene, ubo, W, H)
    fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
    return rig, fi, cur, ubo


def lights_image(ctx, scene, fi, W, H, bias=None):
    import torch
    from hybrid_rendering_amd import lights
    p = lights.Lights(ctx, W, H)
    if bias is not None:
        p.params.bias = bias
    p.render(scene, fi)
    torch.cuda.synchronize()
    img = helpers.bits16(p.output()).copy()
    p.close()
    return img


def composite_image(hr, ctx, rig, fi, W, H):
    """hr_deferred_render with every flag off under a black environment (sky, prefiltered chain and SH9 all 0): the UBO light's unshadowed term alone"""
    import torch
    from hybrid_rendering_amd import api_deferred
    df = api_deferred.DeferredShading(ctx, W, H)
    df.params.use_ray_traced_shadows = df.params.use_ray_traced_ao = df.params.use_ray_traced_reflections = df.params.use_ddgi = 0
    df.render(fi, rig.env)
    torch.cuda.synchronize()
    img = helpers.bits16(df.output()).copy()
    df.close()
    return img


def rebuilt_rays(rig, ubo, cur, L, bias=0.5):
    """The shadow rays of the primary pass for light L, rebuilt on the host: [h][w][8] (origin, t_max, direction, t_min), and for point and spot
    lights two more directions a few float32 ulp to either side.  The origin P + N * bias is the oracle's (orc_shadows_gen_rays writes it for every
    surface texel, whatever the light); P is tests/probe_vis_reference.py's float32 world_pos_from_depth, in the device's order."""
    from oracle import pyoracle as po
    import probe_vis_reference as pv
    h, w = cur["depth"].shape
    origin = po.shadows_gen_rays(ubo, cur["depth"], cur["gb2"], rig.sob, rig.sr, bias, 0).reshape(h, w, 8)[..., 0:3]
    rays = np.zeros((h, w, 8), F)
    rays[..., 0:3], rays[..., 7] = origin, 0.01
    L = np.asarray(L, F)
    if L[12] == 0:
        rays[..., 4:7], rays[..., 3] = L[0:3], 10000.0          # Wi is data0.xyz verbatim: the rebuild is exact
        return [rays]
    x = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    y = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    u, v = np.meshgrid(x, y)
    P = pv.world_pos_from_depth(u.astype(F), v.astype(F), cur["depth"].astype(F), np.asarray(ubo["view_proj_inverse"], F))
    with np.errstate(all="ignore"):
        to_light = (L[4:7] - P).astype(F)
        d2 = ((to_light[..., 0] * to_light[..., 0] + to_light[..., 1] * to_light[..., 1]) + to_light[..., 2] * to_light[..., 2]).astype(F)
        dist = np.sqrt(d2).astype(F)
        Wi = (to_light * (F(1.0) / dist)[..., None]).astype(F)
    rays[..., 4:7], rays[..., 3] = Wi, dist
    out = [rays]
    for sign in (+1.0, -1.0):       # the direction turned by 4e-7 rad about two axes and the reach changed by four ulp: a ray whose answer hangs on the last bits shows
        r = rays.copy()
        r[..., 4:7] = Wi + F(sign * 4e-7) * np.stack([Wi[..., 1], -Wi[..., 2], Wi[..., 0]], -1)
        r[..., 3] = dist * F(1.0 + sign * 5e-7)
        out.append(r)
    return out


@pytest.mark.parametrize("kind,cutout", KINDS)
@pytest.mark.parametrize("W,H", [(lc.W, lc.H), lc.RAGGED])
def test_swap_identity_on_the_primary_surfaces(hr, ctx, kind, cutout, W, H):
    """item 2: black environment, composite flags off.  At every surface texel the hr_lights image under list [L] is bitwise the composite under UBO
    light L, or +0; sky texels are (0, 0, 0, 0), surface texels have alpha 1.  The zero set: where the composite is not 0 (the light reaches the
    texel: attenuation > 0), hr_lights is 0 exactly where hr_trace_any_hit finds an occluder for the rebuilt ray.  Directional: the rebuild is exact
    and the sets are equal.  Point and spot: equal on the texels whose answer does not change when the rebuilt direction is turned by 4e-7 rad and
    its reach changed by 5e-7 (the float32 rebuild of Wi is then unambiguous); how many texels that leaves out is printed and capped at 1 %."""
    import torch
    scene = make(hr, ctx, kind, cutout)
    half, zero = np.float16(1.0).view(np.uint16), 0
    for cam_name, cam in (("inside", lc.camera(W / H)), ("outside", lc.camera_outside(W / H))):
        for which, make_light in lc.LIGHTS.items():
            L = make_light()
            rig, fi_b, cur, ubo_b = primary_setup(hr, ctx, scene, W, H, cam, lc.dark(L))
            _, fi_a, _, ubo_a = primary_setup(hr, ctx, scene, W, H, cam, L)
            comp = composite_image(hr, ctx, rig, fi_a, W, H)
            scene.set_lights(lc.records(L))
            got = lights_image(ctx, scene, fi_b, W, H)
            scene.set_lights([])
            surface = cur["depth"] != 1.0
            assert np.all(got[~surface] == 0), "sky texels are (0, 0, 0, 0)"
            assert np.all(got[surface][:, 3] == half)
            if cam_name == "outside":
                assert (~surface).sum() > 0.2 * W * H
            same = (got[..., :3] == comp[..., :3]).all(-1)
            is_zero = (got[..., :3] == zero).all(-1)                 # +0 bit patterns: a -0 would not pass
            assert np.all((same | is_zero)[surface]), f"{kind} {which} {cam_name}: {int((~(same | is_zero))[surface].sum())} surface texels are neither the composite's bits nor +0"
            reached = surface & (comp[..., :3] != 0).any(-1)
            variants = [scene.any_hit(torch.from_numpy(np.ascontiguousarray(r.reshape(-1, 8))).cuda()).cpu().numpy().reshape(H, W) != 0 for r in rebuilt_rays(rig, ubo_b, cur, L)]
            sure = reached & np.all([v == variants[0] for v in variants], axis=0)
            left_out = int((reached & ~sure).sum())
            print(f"{kind} cutout={cutout} {W}x{H} {which} {cam_name}: {int(reached.sum())} texels reached, {int((is_zero & reached).sum())} shadowed, {left_out} left out as ambiguous")
            if which == "directional":
                assert left_out == 0
            assert left_out <= 0.01 * surface.sum()
            assert np.array_equal(is_zero[sure], variants[0][sure]), f"{kind} {which} {cam_name}: the zero set differs from hr_trace_any_hit on {int((is_zero[sure] != variants[0][sure]).sum())} texels"
            if cam_name == "inside":
                assert reached.sum() > 0.15 * W * H and (is_zero & reached).sum() < reached.sum(), "the light reaches the view"
                if not cutout:
                    assert (is_zero & reached).sum() > 0, "the cubes cast shadows into the view"
    scene.close()


# ---- list order and count -----------------------------------------------------------------------------------------------------------------------------
def test_list_order_and_count_on_the_primary_surfaces(hr, ctx):
    """item 3, primary pass.  Two spots whose cones are disjoint (tests/lights_cases.py disjoint_spots): every texel's sum is +0 plus one term, so
    the image under [a, b] and under [b, a] is the two single-light images combined, bit for bit.
    Three overlapping lights: the image lies within 2 fp16 ulp (at the larger value) of fp16(sum of the float values of the single-light images).
    Derivation for n = 3: a single image is fp16(x_i), off x_i by at most half an fp16 ulp, i.e. at most 2^-11 x_i; the pass sums the x_i in fp32, off
    the exact sum S by at most (n - 1) 2^-24 S; so the sum of the single images is off S by at most 2^-11 S + 2^-23 S, which is at most
    (1 + 2^-12) fp16 ulp at S (an ulp is at least 2^-11 of its value).  Both sides are then rounded to fp16, half an ulp each: the two fp16 values
    are less than 3 ulp apart, and two values of one grid less than 3 ulp apart are at most 2 apart.  (Below the normal range an ulp is absolute,
    2^-24, and the same count holds with the three half-ulps of the singles: 1.5 + 1 < 3.)
    n = 2, 65 and HR_MAX_LIGHTS with all but the lit lights at intensity 0: bit-equal to the lit subset's image."""
    W, H = lc.RAGGED
    scene = make(hr, ctx, "flat", False)
    L0 = lc.dark(lc.point())
    rig, fi, cur, _ = primary_setup(hr, ctx, scene, W, H, lc.camera(W / H), L0)
    surface = cur["depth"] != 1.0

    def image(*lights, recs=None):
        scene.set_lights(lc.records(*lights) if recs is None else recs)
        return lights_image(ctx, scene, fi, W, H)
    a, b = lc.disjoint_spots()
    ia, ib, iab, iba = image(a), image(b), image(a, b), image(b, a)
    lit_a, lit_b = (ia[..., :3] != 0).any(-1), (ib[..., :3] != 0).any(-1)
    assert lit_a.sum() > 20 and lit_b.sum() > 20 and not (lit_a & lit_b).any(), "both cones are in view and share no texel"
    combined = np.where(lit_a[..., None], ia, ib)
    assert np.array_equal(iab, combined) and np.array_equal(iba, combined)
    three = lc.overlapping()
    singles = [image(l) for l in three]
    f16 = lambda bits: bits.view(np.float16).astype(np.float64)
    want = sum(f16(s[..., :3]) for s in singles).astype(np.float16).view(np.uint16)
    got = image(*three)
    overlap = np.sum([(s[..., :3] != 0).any(-1) for s in singles], axis=0)
    d = ulp16_at_larger(got[..., :3][surface], want[surface])
    print(f"overlapping lights: {int((overlap >= 2).sum())} texels under two or more, max distance {d.max():.2f} ulp")
    assert (overlap >= 2).sum() > 0.2 * W * H and d.max() <= 2.0
    assert np.array_equal(image(three[1], three[0], three[2])[..., 3], got[..., 3])
    for n in (2, 65, lc.HR_MAX_LIGHTS):
        lit = three[:2] if n == 2 else three
        recs, at = lc.padded(lit, n)
        assert np.array_equal(image(recs=recs), image(*lit)), f"n = {n}: the lit lights sit at {at}; the lights of intensity 0 add +0"
        assert scene.get_lights().tobytes() == lc.records(*lit).tobytes()
    scene.close()


@pytest.mark.parametrize("kind,cutout", [("flat", False), ("shared", True)])
def test_list_count_in_the_hit_shaders(hr, ctx, kind, cutout):
    """item 3, hit shaders: lists of 2, 65 and HR_MAX_LIGHTS records of which all but the lit ones have intensity 0 give the images of the lit
    subset's list bit for bit (a light of intensity 0 adds ((T * brdf) * attenuation) * 0 = +0), and more rays"""
    three = lc.overlapping()
    scenes = dict(lit2=(make(hr, ctx, kind, cutout).set_lights(lc.records(*three[:2])), lc.dark(three[0])), lit3=(make(hr, ctx, kind, cutout).set_lights(lc.records(*three)), lc.dark(three[0])))
    for n in (2, 65, lc.HR_MAX_LIGHTS):
        scenes[f"n{n}"] = (make(hr, ctx, kind, cutout).set_lights(lc.padded(three[:2] if n == 2 else three, n)[0]), lc.dark(three[0]))
    snap = run_frames(hr, ctx, scenes, 2)[1]
    for n in (2, 65, lc.HR_MAX_LIGHTS):
        base = "lit2" if n == 2 else "lit3"
        assert_equal_snapshots(snap[f"n{n}"], snap[base], f"{kind}: {n} records against the lit subset", keys=IMAGES)
        if n > 3:
            assert snap[f"n{n}"]["gt_rays"] > snap[base]["gt_rays"]
    assert not np.array_equal(snap["lit2"]["ddgi_radiance"], snap["lit3"]["ddgi_radiance"]) and lit_share(snap["lit3"]["ddgi_radiance"]) > 0.3
    for s, _ in scenes.values():
        s.close()


# ---- off is off ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cutout", KINDS)
def test_off_is_off(hr, ctx, kind, cutout):
    """item 4: set_lights(n = 0) after a non-empty list gives every image AND every ray count of a scene that never had a list (the launches are the
    kernels they were); a list of lights that all have intensity 0 gives the same images (its rays are traced and counted).  The primary pass
    writes (0, 0, 0, 1) on every surface texel for each of the three."""
    L = lc.point()
    never = make(hr, ctx, kind, cutout)
    cleared = make(hr, ctx, kind, cutout).set_lights(lc.records(lc.spot(), lc.directional())).set_lights([])
    zeros = make(hr, ctx, kind, cutout).set_lights(lc.padded([], 5)[0])
    assert cleared.get_lights().shape == (0, 4, 4) and zeros.get_lights().shape == (5, 4, 4)
    frames = run_frames(hr, ctx, dict(never=(never, L), cleared=(cleared, L), zeros=(zeros, L)), 2)
    for f, snap in enumerate(frames):
        assert_equal_snapshots(snap["cleared"], snap["never"], f"{kind} frame {f}: a cleared list against no list")
        assert_equal_snapshots(snap["zeros"], snap["never"], f"{kind} frame {f}: lights of intensity 0 against no list", keys=IMAGES)
        assert lit_share(snap["never"]["ddgi_radiance"]) > 0.3
    W, H = lc.RAGGED
    rig, fi, cur, _ = primary_setup(hr, ctx, never, W, H, lc.camera(W / H), L)
    want = np.zeros((H, W, 4), np.uint16)
    want[cur["depth"] != 1.0, 3] = np.float16(1.0).view(np.uint16)
    for tag, s in (("never", never), ("cleared", cleared), ("zeros", zeros)):
        assert np.array_equal(lights_image(ctx, s, fi, W, H), want), tag
    for s in (never, cleared, zeros):
        s.close()


# ---- the device setter ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "shared"])
def test_device_setter_in_a_captured_graph(hr, ctx, kind):
    """item 5: hr_scene_set_lights_device, hr_lights_render and the DDGI trace launch captured into one graph (after one eager run of each); every
    replay takes the records that are in the tensor THEN and equals a scene given the same records through the host form.  The host form is
    refused while the stream captures, and so is the first setter call of a scene (it allocates)."""
    import torch
    from hybrid_rendering_amd import api_gi, lights
    W, H = lc.W, lc.H
    three = lc.overlapping()
    sets = [lc.records(*three), lc.records(lc.spot(25.0, position=(3.0, 7.0, 4.0)), lc.directional(0.5, (0.1, 1.0, 0.4)), lc.point(9.0, (7.0, 4.0, 3.0))),
            lc.records(three[2], three[0], three[1])]
    dev, host, fresh = make(hr, ctx, kind, False).set_lights(sets[0]), make(hr, ctx, kind, False), make(hr, ctx, kind, False)
    rig, fi, cur, ubo = primary_setup(hr, ctx, dev, W, H, lc.camera(W / H), lc.dark(three[0]))
    gi = {tag: api_gi.DDGI(ctx, W, H, rig.ddgi) for tag in ("dev", "host")}
    lp = {tag: lights.Lights(ctx, W, H) for tag in ("dev", "host")}
    for g in gi.values():
        g.params.infinite_bounces = 0

    def run(tag, scene):
        lp[tag].render(scene, fi)
        gi[tag].ray_trace(scene, fi, rig.env)

    def read(tag):
        torch.cuda.synchronize()
        return helpers.bits16(lp[tag].output()).copy(), helpers.bits16(gi[tag].image(gi[tag].IMG_RADIANCE)).copy()
    buf = torch.from_numpy(sets[0]).cuda()
    dev.set_lights_device(buf)
    run("dev", dev)
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(hr.HRError) as e:
            dev.set_lights(sets[1])
        assert "HR_ERR_INVALID_ARG" in str(e.value) and "captur" in str(e.value)
        with pytest.raises(hr.HRError) as e:
            fresh.set_lights_device(buf[:0])         # its list is empty: nothing to copy, but the first call allocates the table
        assert "captur" in str(e.value)
        dev.set_lights_device(buf)
        run("dev", dev)
    assert dev.get_lights().tobytes() == sets[0].tobytes(), "the refused host call changed nothing"
    for k in (1, 2):
        buf.copy_(torch.from_numpy(sets[k]).cuda())
        torch.cuda.synchronize()
        graph.replay()
        got = read("dev")
        host.set_lights(sets[k])
        run("host", host)
        want = read("host")
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{kind}, replay {k}: the device form against the host form"
        assert lit_share(got[0]) > 0.3 and lit_share(got[1]) > 0.3
        if k == 1:
            first = got
    assert not np.array_equal(first[0], got[0]) and not np.array_equal(first[1], got[1]), "the two replays saw different lights"
    for p in list(gi.values()) + list(lp.values()) + [dev, host, fresh]:
        p.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_instrumented_traces_refuse_a_live_list(hr, ctx):
    """item 6: hr_ddgi_trace_stats and hr_reflections_trace_stats return HR_ERR_UNSUPPORTED on a scene with a non-empty list, enqueue nothing, and
    run as ever once the list is cleared; a scene-bound refusal of the setter (n above the cap) leaves the list as it was"""
    import torch
    W, H = lc.W, lc.H
    L = lc.point()
    g = make(hr, ctx, "flat", False).set_lights(lc.records(lc.spot()))
    rig = rig_for(W, H)
    ubo = synth.make_ubo(lc.camera(W / H), None, L)
    cur = all_mirrors(gbuffer_np(g, ubo, W, H))
    fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
    p = Passes(hr, ctx, rig, 1, ground_truth=False)
    before = p.render(g, fi, ubo, synth_env.random_orientation(np.random.RandomState(1)))
    calls = (lambda: p.gi.trace_stats(g, fi, rig.env), lambda: p.refl.trace_stats(g, fi, rig.env, p.gi))
    for stats in calls:
        with pytest.raises(hr.HRError, match="HR_ERR_UNSUPPORTED"):
            stats()
        assert "hr_scene_set_lights" in hr.lib().hr_last_error().decode()
    torch.cuda.synchronize()
    assert_equal_snapshots(p.snapshot(), before, "the refused calls enqueued nothing", keys=("ddgi_radiance", "ddgi_direction_distance", "refl_trace"))
    after = p.render(g, fi, ubo, synth_env.random_orientation(np.random.RandomState(2)))
    assert lit_share(after["refl_trace"]) > 0.3, "the passes are usable after the refusals"
    with pytest.raises(hr.HRError, match="HR_ERR_INVALID_ARG"):
        from hybrid_rendering_amd import lights
        big = np.zeros((257, 4, 4), F)
        lights._check(lights.call("hr_scene_set_lights")(g.h, big.ctypes.data, 257, None), "hr_scene_set_lights")
    assert g.get_lights().shape == (1, 4, 4)
    g.set_lights([])
    for stats in calls:
        assert stats()[0] > 0
    torch.cuda.synchronize()
    p.close(); g.close()


# ---- the hybrid frame -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "shared"])
def test_hybrid_frame_modes_agree_on_a_scene_with_a_list(hr, ctx, kind):
    """item 7: hr_hybrid_frame_render over a scene with a live list, in serial, streams and graph mode, against the four render() calls: DDGI ray
    images and atlases, the reflections trace image and a-trous output, AO and shadows bit for bit, 4 frames with temporal feedback at 64 x 40.  The
    list is cleared for frame 2 and set again for frame 3: the graph mode captures the 5-argument LIGHTS launches, then the plain kernels, then the
    LIGHTS ones again."""
    import torch
    from hybrid_rendering_amd import api_frame
    W, H = lc.W, lc.H
    rig = rig_for(W, H)
    recs = lc.records(lc.spot(), lc.directional(1.0))
    modes = dict(calls=None, serial=api_frame.FRAME_SERIAL, streams=api_frame.FRAME_STREAMS, graph=api_frame.FRAME_GRAPH)
    scenes = {tag: make(hr, ctx, kind, False).set_lights(recs) for tag in modes}
    plain = make(hr, ctx, kind, False)
    sets = {tag: Passes(hr, ctx, rig, 1, ground_truth=False) for tag in list(modes) + ["plain"]}
    for p in sets.values():
        p.gi.params.infinite_bounces = 0      # the probe rays' radiance then holds no history: with the list cleared it is the scene's that never had one
    shadows = {tag: hr.RayTracedShadows(ctx, W, H) for tag in sets}
    native = {tag: api_frame.HybridFrame(ctx, shadows[tag], sets[tag].ao, sets[tag].gi, sets[tag].refl) for tag, mode in modes.items() if mode is not None}
    rng = np.random.RandomState(9)
    light = lc.point()
    prev = None
    for f in range(4):
        live = f != 2
        for s in scenes.values():
            s.set_lights(recs if live else [])
        ubo = synth.make_ubo(lc.camera(W / H), None, light)
        cur = all_mirrors(gbuffer_np(plain, ubo, W, H))
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        snap = {}
        for tag in sets:
            p = sets[tag]
            if tag in native:
                p.gi.set_orientation(orient)
                native[tag].render(scenes[tag], rig.env, fi, fi, fi, fi, mode=modes[tag])
            else:
                scene = plain if tag == "plain" else scenes[tag]
                shadows[tag].render(scene, fi)
                p.render(scene, fi, ubo, orient)
            torch.cuda.synchronize()
            snap[tag] = p.snapshot()
            snap[tag]["shadow_mask"] = shadows[tag].image(shadows[tag].IMG_MASK).cpu().numpy()
        for tag in ("serial", "streams", "graph"):
            assert_equal_snapshots(snap[tag], snap["calls"], f"{kind}, frame {f} (list {'set' if live else 'cleared'}): {tag} mode against the render() calls")
        assert np.array_equal(snap["graph"]["ddgi_radiance"], snap["plain"]["ddgi_radiance"]) == (not live), f"frame {f}: DDGI radiance against the scene without a list"
        assert np.array_equal(snap["graph"]["ddgi_direction_distance"], snap["plain"]["ddgi_direction_distance"]) and np.array_equal(snap["graph"]["shadow_mask"], snap["plain"]["shadow_mask"])
        assert np.array_equal(snap["graph"]["ao_masks"], snap["plain"]["ao_masks"]), "shadows and AO do not read the list"
        prev = cur
    inst, upd = native["graph"].graph_stats()
    assert inst >= 1 and inst + upd == 4
    for n in native.values():
        n.close()
    for p in list(sets.values()) + list(shadows.values()) + list(scenes.values()) + [plain]:
        p.close()


# ---- a second lamp ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_second_lamp_lights_its_half_of_the_room(hr, ctx):
    """item 8: the closed room with a thick wall across x = 5 (lights_cases.partitioned), the UBO light dark, a black sky, one point light of the
    list at x = 2.  After four DDGI frames with infinite bounces every one of the nine probes at x = 1.5 has irradiance, and their mean exceeds
    that of the nine at x = 8.5, behind the wall; with an empty list every probe is black."""
    import torch
    from hybrid_rendering_amd import api_gi
    W, H = lc.W, lc.H
    lamp = lc.point(40.0, position=(2.0, 6.0, 5.0))
    rig = rig_for(W, H, black_sky=True, rays=128)
    ubo = synth.make_ubo(lc.camera(W / H), None, lc.dark(lamp))
    mean = {}
    for tag in ("lamp", "none"):
        g = hr.Scene(ctx, lc.partitioned().flatten())
        if tag == "lamp":
            g.set_lights(lc.records(lamp))
        cur = gbuffer_np(g, ubo, W, H)
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
        gi = api_gi.DDGI(ctx, W, H, rig.ddgi)
        rng = np.random.RandomState(6)
        for f in range(4):
            gi.render(g, fi, rig.env, synth_env.random_orientation(rng))
        torch.cuda.synchronize()
        atlas = helpers.bits16(gi.current_read()[0])
        u = rig.ddgi
        nx, ny, nz = (int(v) for v in u["probe_counts"])
        side = int(u["irradiance_probe_side_length"])
        m = np.zeros(nx * ny * nz)
        for i in range(len(m)):
            col, row = i % (nx * ny), i // (nx * ny)
            cell = atlas[row * (side + 2) + 2:row * (side + 2) + 2 + side, col * (side + 2) + 2:col * (side + 2) + 2 + side, :3]
            m[i] = cell.view(np.float16).astype(np.float64).mean()
        mean[tag] = m.reshape(nz, ny, nx)
        gi.close(); g.close()
    near, behind = mean["lamp"][:, :, 0], mean["lamp"][:, :, nx - 1]
    print(f"mean irradiance of the probes at x = 1.5: {near.mean():.4f}; at x = 8.5: {behind.mean():.4f}")
    assert near.min() > 0 and near.mean() > behind.mean()
    assert not mean["none"].any(), "with an empty list the room stays black"
