"""Alpha-tested cutout materials through every pass that walks a scene (the CUTOUT instantiations of k_shadows_trace, k_ao_trace, k_ddgi_trace,
k_refl_trace, k_ground_truth and k_gbuffer_raycast, on flat and on shared instanced scenes).  The per-texel decision is pinned by
tests/test_gpu_cutout.py; here the passes are checked through whole-triangle equivalences that need no reference at all:
  (a) a cutout material whose texture alpha is 0 everywhere == a scene created without those triangles;
  (b) a cutout material whose alpha is 255 everywhere, cutoff 1.0 == the same scene with no cutoffs set;
and every stage image, mask, ray count and atlas is compared with array_equal on bits.  A walk that forgot the accept test fails (a)."""
import numpy as np
import pytest

import cutout_cases as cc
import helpers
from hybrid_rendering_amd import synth, synth_env
from test_gpu_shared_passes import Passes, Rig, assert_equal_snapshots, gbuffer_np

pytestmark = pytest.mark.gpu

CUT = 1                                              # the material the equivalences turn into a cutout
ONLY_CUT = np.array([0.0, 0.5, 0.0, 0.0], np.float32)
ZEROS = np.zeros(4, np.float32)
VISIBILITY = ("shadow_masks", "shadow_rays", "shadow_atrous", "fast_shadow_masks", "fast_shadow_atrous", "ao_masks", "ao_rays", "ao_denoised")


def cameras(lo, hi, aspect, n):
    c, rad = 0.5 * (np.asarray(lo, np.float64) + hi), 0.5 * float(np.linalg.norm(np.asarray(hi, np.float64) - lo))
    return [synth.Camera(tuple(c + rad * np.array([1.1 + 0.03 * f, 0.45, 0.8 - 0.04 * f])), tuple(c), fov=50.0, aspect=aspect, near=0.02 * rad, far=8.0 * rad) for f in range(n)]


def all_mirrors(cur):
    """gb3.x = 0.03 on every surface pixel: each traces a mirror reflection ray"""
    cur["gb3"][..., 0][cur["depth"] != 1.0] = np.float16(0.03).view(np.uint16)
    return cur


class Set:
    """every pass for ONE scene: AO, DDGI, reflections, ground truth (exact mode) and the shadows pass in both arithmetic modes"""

    def __init__(self, hr, ctx, rig):
        self.hr, self.p = hr, Passes(hr, ctx, rig, 1)
        self.shadows = {exact: hr.RayTracedShadows(ctx, rig.W, rig.H) for exact in (1, 0)}
        for exact, s in self.shadows.items():
            s.params.exact = exact

    def render(self, scene, fi, ubo, orient):
        import torch
        s = self.p.render(scene, fi, ubo, orient)
        for exact, sh in self.shadows.items():
            sh.render(scene, fi)
            torch.cuda.synchronize()
            tag = "" if exact else "fast_"
            s[tag + "shadow_masks"] = sh.image(sh.IMG_MASK).cpu().numpy().view(np.uint32).copy()
            s[tag + "shadow_atrous"] = helpers.bits16(sh.output(self.hr.OUTPUT_ATROUS))
            if exact:
                s["shadow_rays"] = sh.ray_count()
        return s

    def close(self):
        self.p.close()
        for s in self.shadows.values():
            s.close()


def gbuffers(scene, ubo, W, H):
    """the G-buffer of hr_gbuffer_raycast and of hr_gbuffer_raycast_motion"""
    plain = gbuffer_np(scene, ubo, W, H)
    motion = {}
    for k, v in scene.gbuffer(ubo, W, H, motion=True).items():
        a = v.cpu().numpy()
        motion["motion_" + k] = a.view(np.uint16) if a.dtype == np.float16 else a
    return plain, motion


def run(hr, ctx, scenes, lo, hi, W, H, frames=3, input_from=None):
    """`frames` frames with temporal feedback over every scene of `scenes` (tag -> scene): each is rendered from its OWN synthesised G-buffer
    (or from `input_from`'s); returns per frame tag -> snapshot (the passes' images, both G-buffers)"""
    rig = Rig(W, H, lo, hi, probes=(3, 3, 3), rays=32)
    sets = {tag: Set(hr, ctx, rig) for tag in scenes}
    cams, light = cameras(lo, hi, W / H, frames + 1), synth.make_light()
    rng = np.random.RandomState(4)
    prev, out = {}, []
    for s in scenes.values():
        s.motion_begin_frame()
    for f in range(frames):
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        orient = synth_env.random_orientation(rng)
        snap = {}
        gb = {tag: gbuffers(scene, ubo, W, H) for tag, scene in scenes.items()}
        for tag, scene in scenes.items():
            plain, motion = gb[tag]
            cur = all_mirrors({k: v.copy() for k, v in (plain if input_from is None else gb[input_from][0]).items()})
            fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev.get(tag, cur)), ubo, f)
            s = sets[tag].render(scene, fi, ubo, orient)
            s.update({"gbuffer_" + k: v for k, v in plain.items()})
            s.update(motion)
            s["refl_distance"] = s["refl_trace"][..., 3]   # 0.001 + the reflection ray's hit distance (-1: a miss): visibility alone
            snap[tag] = s
            prev[tag] = cur
        out.append(snap)
    for s in sets.values():
        s.close()
    return out


def flat_pair(hr, ctx, alpha, cutoff):
    """(the scene with material CUT on a texture of one alpha value and `cutoff`, the flat scene data behind it)"""
    sd = cc.with_alpha(cc.scene(), CUT, alpha)
    cut = ZEROS.copy()
    cut[CUT] = cutoff
    return hr.Scene(ctx, sd).set_alpha_cutoffs(cut), sd


def shared_pair(hr, ctx, alpha, cutoff):
    isd = cc.with_alpha(cc.instanced(), CUT, alpha)
    cut = ZEROS.copy()
    cut[CUT] = cutoff
    return hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes().set_alpha_cutoffs(cut), isd


@pytest.mark.parametrize("kind", ["flat", "shared"])
@pytest.mark.parametrize("W,H", [(100, 60), (232, 136)])
def test_fully_transparent_material_equals_the_scene_without_it(hr, ctx, kind, W, H):
    """(a): alpha 0 everywhere under cutoff 0.5 — shadows in both arithmetic modes, AO, DDGI, reflections, the ground truth, hr_gbuffer_raycast and
    hr_gbuffer_raycast_motion over 3 frames with temporal feedback, at 100x60 (partial tiles) and 232x136"""
    if kind == "flat":
        x, sd = flat_pair(hr, ctx, 0, 0.5)
        y, z = hr.Scene(ctx, cc.without_material(sd, CUT)), hr.Scene(ctx, sd)
        lo, hi = sd.bounds()
    else:
        x, isd = shared_pair(hr, ctx, 0, 0.5)
        y = hr.InstancedScene(ctx, cc.instanced_without_material(isd, CUT), shared=True).enable_two_level_passes()
        z = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()
        lo, hi = isd.flatten().bounds()
    frames = run(hr, ctx, dict(cutout=x, without=y, opaque=z), lo, hi, W, H)
    for f, snap in enumerate(frames):
        assert_equal_snapshots(snap["cutout"], snap["without"], f"{kind} {W}x{H}, frame {f}: alpha 0 against the scene without the material")
        assert snap["cutout"]["shadow_rays"] > 0 and snap["cutout"]["ao_rays"] > 0 and snap["cutout"]["refl_rays"] > 0
        for k in ("gbuffer_depth", "shadow_masks", "ao_masks", "ddgi_direction_distance", "refl_trace", "ground_truth"):
            assert not np.array_equal(snap["cutout"][k], snap["opaque"][k]), f"{kind}, frame {f}: {k} must see that the material is gone"
    for s in (x, y, z):
        s.close()


@pytest.mark.parametrize("kind", ["flat", "shared"])
@pytest.mark.parametrize("W,H", [(100, 60), (232, 136)])
def test_fully_opaque_cutout_equals_no_cutoffs(hr, ctx, kind, W, H):
    """(b): alpha 255 everywhere under cutoff 1.0 — everything bit-identical to the same scene with no cutoffs set (100x60 and 232x136, 3 frames)"""
    if kind == "flat":
        x, sd = flat_pair(hr, ctx, 255, 1.0)
        y = hr.Scene(ctx, sd)
        lo, hi = sd.bounds()
    else:
        x, isd = shared_pair(hr, ctx, 255, 1.0)
        y = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()
        lo, hi = isd.flatten().bounds()
    for f, snap in enumerate(run(hr, ctx, dict(cutout=x, plain=y), lo, hi, W, H)):
        assert_equal_snapshots(snap["cutout"], snap["plain"], f"{kind} {W}x{H}, frame {f}: alpha 255 under cutoff 1.0 against no cutoffs")
    for s in (x, y):
        s.close()


def test_shared_passes_equal_the_flat_scene_over_the_flattened_vertices(hr, ctx):
    """the per-texel cutouts of tests/test_gpu_cutout.py through the passes whose output is a function of visibility alone — the G-buffer's depth, the
    shadows pass, AO, and the hit distances of the probe rays and the reflection rays — on the shared scene against the flat scene over its flattened vertices, 100x60, 2 frames, both from the flat scene's G-buffer"""
    W, H = 100, 60
    isd = cc.instanced()
    flat = isd.flatten()
    gs = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes().set_alpha_cutoffs(cc.CUTOFFS)
    gf, go = hr.Scene(ctx, flat).set_alpha_cutoffs(cc.CUTOFFS), hr.Scene(ctx, flat)
    lo, hi = flat.bounds()
    for f, snap in enumerate(run(hr, ctx, dict(flat=gf, shared=gs, opaque=go), lo, hi, W, H, frames=2, input_from="flat")):
        assert_equal_snapshots(snap["shared"], snap["flat"], f"frame {f}: shared against flat", keys=VISIBILITY + ("gbuffer_depth", "motion_depth", "ddgi_direction_distance", "refl_distance"))
        for k in ("gbuffer_depth", "shadow_masks", "ao_masks", "ddgi_direction_distance", "refl_distance"):
            assert not np.array_equal(snap["flat"][k], snap["opaque"][k]), f"frame {f}: {k} must meet rejected hits"
    for s in (gs, gf, go):
        s.close()


def test_each_ray_class_follows_its_own_opaque_flag(hr, ctx):
    """cutoffs on; set_ray_class_opaque(cls, 1) makes exactly the rays of cls answer like the untouched scene, through the path that fires them:
    RAY_PRIMARY the G-buffer, RAY_SHADOW the shadows pass (and the light rays inside hit shading), RAY_AO the AO masks, RAY_REFLECTION the trace image's
    hit distances, RAY_GI the probe rays' hit distances.  Every scene is rendered from the opaque scene's G-buffer.  (RAY_QUERY: tests/test_gpu_cutout.py)"""
    W, H = 100, 60
    sd = cc.scene()
    classes = dict(primary=hr.RAY_PRIMARY, shadow=hr.RAY_SHADOW, ao=hr.RAY_AO, reflection=hr.RAY_REFLECTION, gi=hr.RAY_GI)
    scenes = dict(opaque=hr.Scene(ctx, sd), cutout=hr.Scene(ctx, sd).set_alpha_cutoffs(cc.CUTOFFS))
    for tag, cls in classes.items():
        scenes[tag] = hr.Scene(ctx, sd).set_alpha_cutoffs(cc.CUTOFFS).set_ray_class_opaque(cls, True)
    lo, hi = sd.bounds()
    shadows, ao = ("shadow_masks", "shadow_rays", "shadow_atrous", "fast_shadow_masks", "fast_shadow_atrous"), ("ao_masks", "ao_rays", "ao_denoised")
    gbuf = tuple("gbuffer_" + k for k in ("gb1", "gb2", "gb3", "depth")) + tuple("motion_" + k for k in ("gb1", "gb2", "gb3", "depth"))
    own = dict(primary=gbuf, shadow=shadows, ao=ao, reflection=("refl_distance",), gi=("ddgi_direction_distance",))
    for f, snap in enumerate(run(hr, ctx, scenes, lo, hi, W, H, frames=2, input_from="opaque")):
        for keys in own.values():
            for k in keys:
                if not k.endswith("_rays"):
                    assert not np.array_equal(snap["cutout"][k], snap["opaque"][k]), f"frame {f}: {k} must meet rejected hits"
        for tag in classes:
            assert_equal_snapshots(snap[tag], snap["opaque"], f"frame {f}: class {tag} forced opaque, its own path against the untouched scene", keys=own[tag])
            for other, keys in own.items():
                if other != tag:
                    assert_equal_snapshots(snap[tag], snap["cutout"], f"frame {f}: class {tag} forced opaque, the path of {other} against the cutout scene", keys=keys)
    for s in scenes.values():
        s.close()


@pytest.mark.parametrize("kind", ["flat", "shared"])
@pytest.mark.parametrize("W,H", [(100, 60), (232, 136)])
def test_hybrid_frame_streams_and_graph_agree(hr, ctx, kind, W, H):
    """(c): hr_hybrid_frame_render in streams mode and in graph mode on the scene of (a), flat and shared — the graph mode picks its instantiations at
    capture like any other launch — and both equal the scene without the material rendered by the four render() calls; 100x60 and 232x136, 3 frames"""
    import torch
    from hybrid_rendering_amd import api_frame
    if kind == "flat":
        x, sd = flat_pair(hr, ctx, 0, 0.5)
        y = hr.Scene(ctx, cc.without_material(sd, CUT))
        lo, hi = sd.bounds()
    else:
        x, isd = shared_pair(hr, ctx, 0, 0.5)
        y = hr.InstancedScene(ctx, cc.instanced_without_material(isd, CUT), shared=True).enable_two_level_passes()
        lo, hi = isd.flatten().bounds()
    rig = Rig(W, H, lo, hi, probes=(3, 3, 3), rays=32)
    modes = dict(calls=None, streams=api_frame.FRAME_STREAMS, graph=api_frame.FRAME_GRAPH)
    sets, shadows, native = {}, {}, {}
    for tag, mode in modes.items():
        sets[tag], shadows[tag] = Passes(hr, ctx, rig, 1, ground_truth=False), hr.RayTracedShadows(ctx, W, H)
        if mode is not None:
            native[tag] = api_frame.HybridFrame(ctx, shadows[tag], sets[tag].ao, sets[tag].gi, sets[tag].refl)
    cams, light = cameras(lo, hi, W / H, 4), synth.make_light()
    rng = np.random.RandomState(9)
    prev = None
    for f in range(3):
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = all_mirrors(gbuffer_np(y, ubo, W, H))
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        snap = {}
        for tag, mode in modes.items():
            p = sets[tag]
            if mode is None:
                shadows[tag].render(y, fi)
                p.render(y, fi, ubo, orient)
            else:
                p.gi.set_orientation(orient)
                native[tag].render(x, rig.env, fi, fi, fi, fi, mode=mode)
            torch.cuda.synchronize()
            snap[tag] = p.snapshot()
            snap[tag]["shadow_mask"] = shadows[tag].image(shadows[tag].IMG_MASK).cpu().numpy()
            snap[tag]["shadows_denoised"] = helpers.bits16(shadows[tag].output(hr.OUTPUT_ATROUS))
        assert_equal_snapshots(snap["streams"], snap["graph"], f"{kind} {W}x{H}, frame {f}: streams against graph")
        assert snap["graph"]["ao_rays"] > 0 and snap["graph"]["refl_rays"] > 0
        assert_equal_snapshots(snap["graph"], snap["calls"], f"{kind} {W}x{H}, frame {f}: the hybrid frame on the cutout scene against render() calls on the scene without the material")
        prev = cur
    for n in native.values():
        n.close()
    for p in list(sets.values()) + list(shadows.values()) + [x, y]:
        p.close()


def test_the_occluder_cache_holds_no_rejected_triangle(hr, ctx):
    """shadows pass, 3 frames, default cache on; between frames 1 and 2 material CUT turns from opaque to fully transparent: frame 2's mask equals that
    of a newly created pass given the same inputs, and differs from frame 2 of the scene left opaque (the cached occluders of the material were in use)"""
    import torch
    W, H = 100, 60
    sd = cc.with_alpha(cc.scene(), CUT, 0)
    g, still = hr.Scene(ctx, sd), hr.Scene(ctx, sd)
    lo, hi = sd.bounds()
    rig = Rig(W, H, lo, hi)
    cams, light = cameras(lo, hi, W / H, 4), synth.make_light()
    p, q = hr.RayTracedShadows(ctx, W, H), hr.RayTracedShadows(ctx, W, H)
    prev = None
    for f in range(3):
        if f == 2:
            g.set_alpha_cutoffs(ONLY_CUT)
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = gbuffer_np(still, ubo, W, H)
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        p.render(g, fi); q.render(still, fi)
        torch.cuda.synchronize()
        prev = cur
    fresh = hr.RayTracedShadows(ctx, W, H)
    fresh.ray_trace(g, fi)
    torch.cuda.synchronize()
    mask = lambda s: s.image(s.IMG_MASK).cpu().numpy().view(np.uint32)
    assert np.array_equal(mask(p), mask(fresh)), "frame 2 of the pass that cached occluders of the material against a newly created pass"
    assert not np.array_equal(mask(p), mask(q)), "the material cast shadows while it was opaque"
    for s in (p, q, fresh, g, still):
        s.close()


def test_instrumented_traces_refuse_a_cutout_scene(hr, ctx):
    """hr_shadows_trace_stats and hr_ao_trace_stats refuse a scene whose cutouts are enabled for their class, before anything is enqueued, and take it
    again with the class forced opaque or every cutoff 0"""
    import torch
    W, H = 100, 60
    sd = cc.scene()
    g = hr.Scene(ctx, sd).set_alpha_cutoffs(cc.CUTOFFS)
    lo, hi = sd.bounds()
    rig = Rig(W, H, lo, hi)
    ubo = synth.make_ubo(cameras(lo, hi, W / H, 1)[0], None, synth.make_light())
    cur = gbuffer_np(g, ubo, W, H)
    fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
    sh, ao = hr.RayTracedShadows(ctx, W, H), hr.RayTracedAO(ctx, W, H, 0)
    sh.render(g, fi); ao.render(g, fi)
    torch.cuda.synchronize()
    before = sh.image(sh.IMG_MASK).cpu().numpy().copy(), ao.image(ao.IMG_MASK).cpu().numpy().copy()
    for p, cls in ((sh, hr.RAY_SHADOW), (ao, hr.RAY_AO)):
        with pytest.raises(hr.HRError, match="HR_ERR_UNSUPPORTED"):
            p.trace_stats(g, fi)
        assert "alpha cutoffs" in hr.lib().hr_last_error().decode()
        g.set_ray_class_opaque(cls, True)
        p.trace_stats(g, fi)
        g.set_ray_class_opaque(cls, False)
    torch.cuda.synchronize()
    g.set_alpha_cutoffs(ZEROS)
    sh.trace_stats(g, fi); ao.trace_stats(g, fi)
    g.set_alpha_cutoffs(cc.CUTOFFS)
    sh.ray_trace(g, fi); ao.ray_trace(g, fi)
    torch.cuda.synchronize()
    assert np.array_equal(sh.image(sh.IMG_MASK).cpu().numpy(), before[0]) and np.array_equal(ao.image(ao.IMG_MASK).cpu().numpy(), before[1])
    for s in (sh, ao, g):
        s.close()


def test_light_rays_inside_hit_shading_and_the_ground_truth_follow_the_flags(hr, ctx):
    """the kernels that fire several classes get one view per class (DDGI: GI + SHADOW; reflections: REFLECTION + SHADOW; ground truth: PRIMARY + SHADOW,
    and GI for its bounces).  `all`: every class those kernels fire forced opaque — DDGI's images and atlases, the whole reflections trace image and the
    ground truth equal the untouched scene's while AO, not forced, keeps the cutout answer.  `but_shadow`: the same without RAY_SHADOW — the rays' own
    hit distances still equal the untouched scene's, and the colours, which hold the light and sky rays, equal neither scene's.  `only_shadow`: the
    reverse.  `only_gi`: the direct-only ground truth fires no GI ray and must equal the cutout scene's.  100x60, 2 frames, the opaque scene's G-buffer."""
    W, H = 100, 60
    sd = cc.scene()
    force = dict(all=("PRIMARY", "SHADOW", "REFLECTION", "GI"), but_shadow=("PRIMARY", "REFLECTION", "GI"), only_shadow=("SHADOW",), only_gi=("GI",))
    scenes = dict(opaque=hr.Scene(ctx, sd), cutout=hr.Scene(ctx, sd).set_alpha_cutoffs(cc.CUTOFFS))
    for tag, classes in force.items():
        scenes[tag] = hr.Scene(ctx, sd).set_alpha_cutoffs(cc.CUTOFFS)
        for c in classes:
            scenes[tag].set_ray_class_opaque(getattr(hr, "RAY_" + c), True)
    lo, hi = sd.bounds()
    ddgi = ("ddgi_radiance", "ddgi_direction_distance", "ddgi_irradiance", "ddgi_depth")
    shaded = ("ddgi_radiance", "refl_trace", "ground_truth")
    for f, snap in enumerate(run(hr, ctx, scenes, lo, hi, W, H, frames=2, input_from="opaque")):
        o, c = snap["opaque"], snap["cutout"]
        for k in shaded + ("ddgi_direction_distance", "refl_distance", "ao_masks", "shadow_masks"):
            assert not np.array_equal(o[k], c[k]), f"frame {f}: {k} must meet rejected hits"
        assert_equal_snapshots(snap["all"], o, f"frame {f}: every class of the hit-shading kernels forced opaque", keys=ddgi + ("refl_trace", "refl_rays", "refl_atrous", "ground_truth", "shadow_masks"))
        assert_equal_snapshots(snap["all"], c, f"frame {f}: RAY_AO is not forced", keys=("ao_masks", "ao_rays", "ao_denoised"))
        assert_equal_snapshots(snap["but_shadow"], o, f"frame {f}: the rays' own hits with their classes forced opaque", keys=("ddgi_direction_distance", "refl_distance"))
        assert_equal_snapshots(snap["but_shadow"], c, f"frame {f}: RAY_SHADOW is not forced", keys=("shadow_masks", "shadow_rays"))
        assert_equal_snapshots(snap["only_shadow"], c, f"frame {f}: the rays' own hits run the test", keys=("ddgi_direction_distance", "refl_distance", "ao_masks"))
        assert_equal_snapshots(snap["only_shadow"], o, f"frame {f}: RAY_SHADOW forced opaque", keys=("shadow_masks", "shadow_rays"))
        for tag in ("but_shadow", "only_shadow"):
            for k in shaded:
                assert not np.array_equal(snap[tag][k], o[k]) and not np.array_equal(snap[tag][k], c[k]), f"frame {f}, {tag}: {k} holds light rays of one kind and own rays of the other"
        assert_equal_snapshots(snap["only_gi"], c, f"frame {f}: the direct-only ground truth fires no RAY_GI ray", keys=("ground_truth", "shadow_masks", "refl_distance"))
        assert_equal_snapshots(snap["only_gi"], o, f"frame {f}: the probe rays with RAY_GI forced opaque", keys=("ddgi_direction_distance",))
    for s in scenes.values():
        s.close()


def test_ground_truth_bounces_follow_ray_gi(hr, ctx):
    """trace_indirect = 1: the bounces are class RAY_GI.  With PRIMARY, SHADOW and GI forced opaque the image is the untouched scene's; with GI left to the
    alpha test it is neither the untouched nor the cutout scene's; with only GI forced it is neither as well"""
    import torch
    from hybrid_rendering_amd import api_post
    W, H = 100, 60
    sd = cc.scene()
    lo, hi = sd.bounds()
    rig = Rig(W, H, lo, hi)
    ubo = synth.make_ubo(cameras(lo, hi, W / H, 1)[0], None, synth.make_light())
    force = dict(opaque=None, cutout=(), all=("PRIMARY", "SHADOW", "GI"), but_gi=("PRIMARY", "SHADOW"), only_gi=("GI",))
    img = {}
    for tag, classes in force.items():
        g = hr.Scene(ctx, sd)
        if classes is not None:
            g.set_alpha_cutoffs(cc.CUTOFFS)
            for c in classes:
                g.set_ray_class_opaque(getattr(hr, "RAY_" + c), True)
        gt = api_post.GroundTruthPathTracer(ctx, W, H)
        gt.params.trace_indirect, gt.params.max_ray_bounces = 1, 3
        gt.render(g, ubo, rig.env)
        torch.cuda.synchronize()
        img[tag] = helpers.bits16(gt.output())
        gt.close(); g.close()
    assert not np.array_equal(img["opaque"], img["cutout"])
    assert np.array_equal(img["all"], img["opaque"]), "PRIMARY, SHADOW and GI forced opaque"
    for tag in ("but_gi", "only_gi"):
        assert not np.array_equal(img[tag], img["opaque"]) and not np.array_equal(img[tag], img["cutout"]), tag


def test_instrumented_ddgi_and_reflections_refuse_a_cutout_scene(hr, ctx):
    """hr_ddgi_trace_stats and hr_reflections_trace_stats fire two classes each (their own and RAY_SHADOW): they refuse while EITHER runs the alpha test,
    before anything is enqueued, and run with both forced opaque or every cutoff 0"""
    import torch
    W, H = 100, 60
    sd = cc.scene()
    g = hr.Scene(ctx, sd).set_alpha_cutoffs(cc.CUTOFFS)
    lo, hi = sd.bounds()
    rig = Rig(W, H, lo, hi)
    ubo = synth.make_ubo(cameras(lo, hi, W / H, 1)[0], None, synth.make_light())
    cur = all_mirrors(gbuffer_np(g, ubo, W, H))
    fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
    p = Passes(hr, ctx, rig, 1, ground_truth=False)
    before = p.render(g, fi, ubo, synth_env.random_orientation(np.random.RandomState(1)))
    calls = ((hr.RAY_GI, lambda: p.gi.trace_stats(g, fi, rig.env)), (hr.RAY_REFLECTION, lambda: p.refl.trace_stats(g, fi, rig.env, p.gi)))
    for own, stats in calls:
        for forced in ((), (own,), (hr.RAY_SHADOW,)):
            for c in forced:
                g.set_ray_class_opaque(c, True)
            with pytest.raises(hr.HRError, match="HR_ERR_UNSUPPORTED"):
                stats()
            assert "alpha cutoffs" in hr.lib().hr_last_error().decode()
            for c in forced:
                g.set_ray_class_opaque(c, False)
    torch.cuda.synchronize()
    after = p.snapshot()
    assert_equal_snapshots(after, before, "the refused calls enqueued nothing", keys=("ddgi_radiance", "ddgi_direction_distance", "refl_trace"))
    for own, stats in calls:
        g.set_ray_class_opaque(own, True).set_ray_class_opaque(hr.RAY_SHADOW, True)
        assert stats()[0] > 0
        g.set_ray_class_opaque(own, False).set_ray_class_opaque(hr.RAY_SHADOW, False)
    g.set_alpha_cutoffs(ZEROS)
    for own, stats in calls:
        assert stats()[0] > 0
    torch.cuda.synchronize()
    p.close(); g.close()
