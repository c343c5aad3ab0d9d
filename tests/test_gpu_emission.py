"""Emissive materials on the GPU (include/hr_emission.h): the raw query against tests/emission_reference.py bit for bit, the emissive image of the
primary hits, and the EMISSIVE instantiations of k_ddgi_trace, k_refl_trace and k_ground_truth through equivalences that need no reference — dark
equals off, a black scene shows E alone, a lit scene shows off + E — on a flat, a private-copy instanced and a shared instanced scene over the same
world-space triangles (tests/emission_cases.py).  The rays of the DDGI and reflection kernels are rebuilt by the oracle's gen_rays (their fp32
directions: IMG_DIRDIST holds them rounded to fp16, which cannot give a textured hit's u, v back bit for bit) and checked against IMG_DIRDIST."""
import numpy as np
import pytest

import emission_cases as ec
import emission_reference as er
import helpers
from hybrid_rendering_amd import synth, synth_env
from test_gpu_shared_passes import Passes, Rig, assert_equal_snapshots, gbuffer_np

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = ("flat", "private", "shared")


def make(hr, ctx, isd, kind):
    if kind == "flat":
        return hr.Scene(ctx, isd.flatten())
    if kind == "private":
        return hr.InstancedScene(ctx, isd)
    return hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()


def rig_for(W, H, black_sky=False, rays=ec.RAYS_PER_PROBE):
    import torch
    from hybrid_rendering_amd import api_gi
    rig = Rig(W, H, (1.5, 1.5, 1.5), (5.0, 5.0, 5.0), probes=ec.PROBES, rays=rays)
    assert rig.ddgi.tobytes() == ec.ddgi_grid(rays=rays).tobytes()
    if black_sky:
        rig.sky, rig.pre = np.zeros_like(rig.sky), np.zeros_like(rig.pre)
        f16 = lambda a: torch.from_numpy(a).cuda().view(torch.float16)
        rig.env = api_gi.environment(f16(rig.sky), f16(rig.pre), 16, 5, f16(rig.lut))
        rig.env_np = dict(sky=rig.sky, prefiltered=rig.pre, pre_size=16, pre_levels=5, lut=rig.lut)
    return rig


def query(scene, rays_np):
    """(prim int32 [n], tuv float32 [n][3]) numpy, and the cuda tensors, of hr_trace_closest_hit"""
    import torch
    tuv, prim = scene.closest_hit(torch.from_numpy(np.ascontiguousarray(rays_np.reshape(-1, 8))).cuda())
    torch.cuda.synchronize()
    return prim, tuv


def emission_of(scene, rays_np):
    """E float32 [n][3] (numpy) of the closest hits of `rays_np`, by hr_trace_closest_hit + hr_scene_emission"""
    import torch
    prim, tuv = query(scene, rays_np)
    E = scene.emission(prim, tuv)
    torch.cuda.synchronize()
    return E.cpu().numpy(), prim.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_query_equals_the_reference_bit_for_bit(hr, ctx, kind):
    """item 1: ~4100 hits of hr_trace_closest_hit plus the crafted ones; constant and textured emitters, scale 1 and 3.7, after set_emissive and
    set_emissive_device; 0 on misses and dark materials"""
    import torch
    isd = ec.instanced()
    g = make(hr, ctx, isd, kind)
    prim_d, tuv_d = query(g, ec.rays())
    cprim, ctuv = ec.crafted_hits(isd)
    prim_d = torch.cat([prim_d, torch.from_numpy(cprim).cuda()])
    tuv_d = torch.cat([tuv_d, torch.from_numpy(ctuv).cuda()])
    prim, tuv = prim_d.cpu().numpy(), tuv_d.cpu().numpy()
    assert (prim < 0).sum() > 100 and (prim >= 0).sum() > 2500

    def check(rgb, tex, scale, what):
        got = g.emission(prim_d, tuv_d).cpu().numpy()
        want, on = ec.expected(isd, rgb, tex, scale, prim, tuv)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{kind}, {what}: {(got != want).any(1).sum()} hits differ"
        assert np.all(got[~on] == 0) and on.sum() > 200
        return got

    assert np.all(g.emission(prim_d, tuv_d).cpu().numpy() == 0), "before the first setter call nothing emits"
    rgb0 = ec.emissive_rgb(isd)
    g.set_emission(True, 1.0)
    assert g.emission_state() == (True, 1.0)
    a = check(rgb0, ec.NO_TEX, 1.0, "constants of the description, scale 1")
    g.set_emissive_textures(ec.EMISSIVE_TEX)
    b = check(rgb0, ec.EMISSIVE_TEX, 1.0, "textured, scale 1")
    assert not np.array_equal(a, b)
    g.set_emission(True, 3.7)
    check(rgb0, ec.EMISSIVE_TEX, 3.7, "textured, scale 3.7")
    rgb1 = np.random.RandomState(3).uniform(0, 4, rgb0.shape).astype(F)
    rgb1[0] = 0                                                   # the walls stay dark
    g.set_emissive(rgb1)
    check(rgb1, ec.EMISSIVE_TEX, 3.7, "after set_emissive")
    rgb2 = (rgb1 * F(0.37)).astype(F)
    g.set_emissive(torch.from_numpy(rgb2).cuda())
    check(rgb2, ec.EMISSIVE_TEX, 3.7, "after set_emissive_device")
    g.set_emissive_textures(ec.NO_TEX).set_emission(False, 1.0)
    check(rgb2, ec.NO_TEX, 1.0, "constants again; the query does not depend on the switch")
    # refusals that need a scene
    for bad, word in (([0] * ec.N_MATERIALS, None), ([3] + [-1] * (ec.N_MATERIALS - 1), "outside the scene's 3 textures"), ([-2] + [-1] * (ec.N_MATERIALS - 1), "below -1")):
        if word is None:
            g.set_emissive_textures(bad).set_emissive_textures(ec.NO_TEX)
        else:
            with pytest.raises(hr.HRError, match="HR_ERR_INVALID_ARG"):
                g.set_emissive_textures(bad)
            assert word in hr.lib().hr_last_error().decode()
    neg = rgb2.copy(); neg[2, 1] = -1.0
    with pytest.raises(hr.HRError, match="HR_ERR_INVALID_ARG"):
        g.set_emissive(neg)
    assert "rgb[2]" in hr.lib().hr_last_error().decode()
    g.close()


def test_enabling_validates_the_constants_of_the_description(hr, ctx):
    """a negative or non-finite emissive component is accepted at creation and while emission is off; enabling names the material"""
    isd = ec.instanced()
    for value in (-0.5, np.inf, np.nan):
        m = np.asarray(isd.materials, F).copy()
        m[3, 6] = value
        import dataclasses
        g = hr.Scene(ctx, dataclasses.replace(isd.flatten(), materials=m))
        g.set_emission(False, 2.0)
        with pytest.raises(hr.HRError, match="HR_ERR_INVALID_ARG"):
            g.set_emission(True, 1.0)
        assert "material 3" in hr.lib().hr_last_error().decode() and g.emission_state() == (False, 2.0)
        g.close()


def emissive_bits(scene, ubo, W, H):
    import torch
    img = scene.emissive_image(ubo, W, H)
    torch.cuda.synchronize()
    return helpers.bits16(img)


@pytest.mark.parametrize("W,H", [(61, 37), (1, 1)])
def test_emissive_image(hr, ctx, W, H):
    """item 2: a table lookup by the G-buffer's mesh id, zero exactly where depth == 1, a primary-class cutout hides the emitter, the kinds agree"""
    isd = ec.instanced()
    rgb, table = ec.per_mesh_id_rgb()
    light = ec.light()
    for cam in (ec.camera(W / H), ec.camera_outside(W / H)):
        ubo = synth.make_ubo(cam, None, light)
        images = {}
        for kind in KINDS:
            g = make(hr, ctx, isd, kind).set_emission(True, 1.0).set_emissive(rgb)
            gb = gbuffer_np(g, ubo, W, H)
            img = emissive_bits(g, ubo, W, H)
            ids = gb["gb3"][..., 2].view(np.float16).astype(np.int32)
            want = np.zeros((H, W, 4), np.uint16)
            surface = gb["depth"] != 1.0
            for mid, c in table.items():
                sel = surface & (ids == mid)
                want[sel, :3] = er.fp16_bits(c)
                want[sel, 3] = np.float16(1.0).view(np.uint16)
            assert np.array_equal(img, want), f"{kind} {W}x{H}: {(img != want).any(-1).sum()} texels differ from the lookup by mesh id"
            assert np.array_equal((img == 0).all(-1), ~surface), "zero exactly where the G-buffer has sky"
            images[kind] = img
            g.close()
        assert np.array_equal(images["flat"], images["private"]) and np.array_equal(images["flat"], images["shared"])
        if W > 1 and cam.eye[2] < ec.S:      # from inside: the room, the cubes, the emitter and the quad each with their colour
            assert len(np.unique(images["flat"].reshape(-1, 4), axis=0)) >= 4
    # a cutout of the primary class hides the emitter: the image of the scene created without that triangle
    ubo = synth.make_ubo(ec.camera(W / H), None, light)
    hidden, without = ec.with_hidden_material(isd, ec.EMITTER), ec.without_material(isd, ec.EMITTER)
    for kind in ("flat", "shared"):
        a = make(hr, ctx, hidden, kind).set_emission(True, 1.0).set_emissive(rgb).set_alpha_cutoffs(ec.cutoffs_for(ec.EMITTER))
        b = make(hr, ctx, without, kind).set_emission(True, 1.0).set_emissive(rgb)
        c = make(hr, ctx, hidden, kind).set_emission(True, 1.0).set_emissive(rgb).set_alpha_cutoffs(ec.cutoffs_for(ec.EMITTER)).set_ray_class_opaque(hr.RAY_PRIMARY, True)
        ia, ib, ic = (emissive_bits(s, ubo, W, H) for s in (a, b, c))
        assert np.array_equal(ia, ib), f"{kind}: the hidden emitter against the scene without it"
        if W > 1:
            assert not np.array_equal(ia, ic), f"{kind}: with the primary class forced opaque the emitter is back"
        for s in (a, b, c):
            s.close()


def run_frames(hr, ctx, scenes, W, H, frames, light, black_sky=False, indirect_gt=True, setup=None):
    """`frames` frames with temporal feedback of every pass over every scene (tag -> scene), all from the first scene's G-buffer; per frame tag -> snapshot"""
    import torch
    from hybrid_rendering_amd import api_post
    rig = rig_for(W, H, black_sky)
    sets = {tag: Passes(hr, ctx, rig, 1) for tag in scenes}
    gt1 = {tag: api_post.GroundTruthPathTracer(ctx, W, H) for tag in scenes} if indirect_gt else {}
    for p in gt1.values():
        p.params.trace_indirect, p.params.max_ray_bounces = 1, 3
    if setup:
        for p in sets.values():
            setup(p)
    rng = np.random.RandomState(4)
    first = next(iter(scenes.values()))
    out, prev = [], None
    for f in range(frames):
        ubo = synth.make_ubo(ec.camera(W / H), None, light)
        cur = ec.all_mirrors(gbuffer_np(first, ubo, W, H))
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        snap = {}
        for tag, scene in scenes.items():
            snap[tag] = sets[tag].render(scene, fi, ubo, orient)
            if indirect_gt:
                gt1[tag].render(scene, ubo, rig.env)
                torch.cuda.synchronize()
                snap[tag]["ground_truth_indirect"] = helpers.bits16(gt1[tag].output())
                snap[tag]["ground_truth_indirect_rays"] = gt1[tag].ray_count()
            snap[tag]["ddgi_rays"] = sets[tag].gi.ray_count() if hasattr(sets[tag].gi, "ray_count") else 0
        out.append(dict(snap=snap, ubo=ubo, cur=cur, orient=orient, f=f))
        prev = cur
    for p in list(sets.values()) + list(gt1.values()):
        p.close()
    return out, rig


@pytest.mark.parametrize("kind", KINDS)
def test_dark_equals_off(hr, ctx, kind):
    """item 3: emission enabled with every constant 0 and no emissive texture — through the host form (the plain kernels are picked) and through
    the device form (the host cannot know: the EMISSIVE kernels run and add nothing) — 3 frames of DDGI (3 x 3 x 3 probes, 32 rays), reflections
    (64 x 40) and the ground truth (trace_indirect 0 and 1): every image, atlas and ray count equals the scene with emission off"""
    import torch
    isd = ec.instanced(emissive=False)
    zeros = np.zeros((ec.N_MATERIALS, 3), F)
    scenes = dict(off=make(hr, ctx, isd, kind), dark_host=make(hr, ctx, isd, kind).set_emission(True, 3.7),
                  dark_device=make(hr, ctx, isd, kind).set_emission(True, 3.7).set_emissive(torch.from_numpy(zeros).cuda()))
    frames, _ = run_frames(hr, ctx, scenes, ec.REFL_W, ec.REFL_H, 3, ec.light())
    for fr in frames:
        for tag in ("dark_host", "dark_device"):
            assert_equal_snapshots(fr["snap"][tag], fr["snap"]["off"], f"{kind}, frame {fr['f']}: {tag} against emission off")
        assert fr["snap"]["off"]["refl_rays"] > 0 and (fr["snap"]["off"]["ddgi_radiance"] != 0).any()
    for s in scenes.values():
        s.close()


def ddgi_rays(rig, orient):
    from oracle import pyoracle_ddgi as od
    return od.gen_rays(rig.ddgi, orient)       # [probes][rays][8]


def refl_rays(rig, refl, fr):
    """([H][W][8] rays of the traced texels' closest-hit batch, traced [H][W]) of the reflections trace launch of frame `fr`"""
    from oracle import pyoracle_reflections as orf
    p = refl.params
    tp = orf.TraceParams(p.bias, p.trim, fr["f"], int(p.sample_gi), int(p.approximate_with_ddgi), p.gi_intensity, p.rough_ddgi_intensity, p.ibl_indirect_specular_intensity)
    H, W = fr["cur"]["depth"].shape
    r = orf.gen_rays(fr["ubo"], fr["cur"], rig.sob, rig.sr, tp)[:H, :W]
    rays = np.zeros((H, W, 8), F)
    rays[..., 0:3], rays[..., 4:7], rays[..., 3], rays[..., 7] = r[..., 0:3], r[..., 4:7], 10000.0, 0.001
    return rays, r[..., 7] != 0


@pytest.mark.parametrize("kind", KINDS)
def test_black_scene_shows_the_emission_alone(hr, ctx, kind):
    """item 4: every albedo 0, light intensity 0, a black sky, infinite_bounces and sample_gi off.  DDGI radiance of every ray that hits ==
    fp16(E of its hit), the reflections trace image == fp16(min(E, 0.7)) on traced texels, the ground truth's frame 0 == fp16(min(E, 1)) at pixels
    whose 2 x 2 block of centre rays lies on one constant emitter"""
    W, H = ec.REFL_W, ec.REFL_H
    isd = ec.black(ec.instanced())
    g = make(hr, ctx, isd, kind).set_emission(True, 1.0).set_emissive_textures(ec.EMISSIVE_TEX)

    def setup(p):
        p.gi.params.infinite_bounces = 0
        p.refl.params.sample_gi = 0
    frames, rig = run_frames(hr, ctx, dict(on=g), W, H, 1, ec.light(0.0), black_sky=True, indirect_gt=False, setup=setup)
    fr, s = frames[0], frames[0]["snap"]["on"]
    # DDGI
    rays = ddgi_rays(rig, fr["orient"])
    assert np.array_equal(s["ddgi_direction_distance"][..., :3], rays[..., 4:7].astype(np.float16).view(np.uint16)), "the rebuilt rays are the rays the kernel traced"
    E, prim = emission_of(g, rays)
    hit = prim >= 0
    got = s["ddgi_radiance"].reshape(-1, 4)[:, :3]
    assert hit.all() and (E != 0).any(1).sum() > 20
    assert np.array_equal(got[hit], er.fp16_bits(E[hit])), f"{kind}: DDGI radiance of {(got[hit] != er.fp16_bits(E[hit])).any(1).sum()} rays is not fp16(E)"
    # reflections
    p = Passes(hr, ctx, rig, 1, ground_truth=False)
    setup(p)
    rays, traced = refl_rays(rig, p.refl, fr)
    p.close()
    E, prim = emission_of(g, rays)
    E, prim = E.reshape(H, W, 3), prim.reshape(H, W)
    want = er.fp16_bits(np.minimum(E, F(0.7)))
    assert traced.sum() > 0.9 * W * H and (E[traced] != 0).any(-1).sum() > 20
    assert np.array_equal(s["refl_trace"][..., :3][traced], want[traced]), f"{kind}: the reflections trace image is not fp16(min(E, 0.7))"
    # ground truth, constants only (the jittered ray's u, v are not known): its own scene, no emissive texture
    gc = make(hr, ctx, isd, kind).set_emission(True, 1.0)
    from hybrid_rendering_amd import api_post
    import torch
    gt = api_post.GroundTruthPathTracer(ctx, W, H)
    gt.render(gc, fr["ubo"], rig.env)
    torch.cuda.synchronize()
    img = helpers.bits16(gt.output())
    ids = gbuffer_np(gc, fr["ubo"], W, H)["gb3"][..., 2].view(np.float16).astype(np.int32)
    rgb = ec.emissive_rgb(isd)
    checked = 0
    for mid, mat in ((4, ec.EMITTER), (5, ec.QUAD)):
        m = ids == mid
        block = np.zeros_like(m)
        block[:-1, :-1] = m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]
        assert block.sum() >= 3
        assert np.all(img[block][:, :3] == er.fp16_bits(np.minimum(rgb[mat], F(1.0)))), f"{kind}: ground truth on mesh id {mid}"
        checked += int(block.sum())
    assert checked >= 6
    # the textured path at depth 0: the quad on a texture of one colour whose texels are 0 or 255 — the bilinear blend of equal texels 0 or 1 is exact
    # ((1 - f) + f rounds to 1) — so E = scale * (1, 0, 1) whatever the jittered ray's u, v
    import dataclasses
    uniform = np.zeros((2, 3, 4), np.uint8)
    uniform[..., 0] = uniform[..., 2] = uniform[..., 3] = 255
    tex = ec.NO_TEX.copy()
    tex[ec.QUAD] = len(isd.textures)
    gu = make(hr, ctx, dataclasses.replace(isd, textures=list(isd.textures) + [uniform]), kind).set_emission(True, 0.75).set_emissive_textures(tex)
    gt.restart_accumulation()
    gt.render(gu, fr["ubo"], rig.env)
    torch.cuda.synchronize()
    direct = helpers.bits16(gt.output())
    for mid, want in ((5, F([0.75, 0.0, 0.75])), (4, np.minimum(F(0.75) * rgb[ec.EMITTER], F(1.0)))):
        m = ids == mid
        block = np.zeros_like(m)
        block[:-1, :-1] = m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]
        assert np.all(direct[block][:, :3] == er.fp16_bits(want)), f"{kind}: ground truth, textured emitter, mesh id {mid}"
    # trace_indirect = 1.  In the black world the throughput after a bounce is a few percent (F0 = 0.04) and the Russian roulette ends nearly every
    # path, so the bounces are checked in the world with its albedos back, still under light intensity 0 and the black sky: the direct terms are 0
    # there too, every term of the chain is T * E >= 0 on top of the same depth-0 term (same jitter, same hit), and fp32 addition, min(., 1) and
    # the fp16 store are monotone: no pixel is darker than the direct-only image, and the bounces reach some
    white = ec.instanced()
    gw = make(hr, ctx, dataclasses.replace(white, textures=list(white.textures) + [uniform]), kind).set_emission(True, 0.75).set_emissive_textures(tex)
    gt.restart_accumulation()
    gt.render(gw, fr["ubo"], rig.env)
    gt1 = api_post.GroundTruthPathTracer(ctx, W, H)
    gt1.params.trace_indirect, gt1.params.max_ray_bounces = 1, 3
    gt1.render(gw, fr["ubo"], rig.env)
    torch.cuda.synchronize()
    direct, indirect = helpers.bits16(gt.output()), helpers.bits16(gt1.output())
    a, b = indirect[..., :3].view(np.float16).astype(F), direct[..., :3].view(np.float16).astype(F)
    nan = np.isnan(a)      # a throughput of 0 / 0 (a sampled direction with pdf 0) is the path tracer's own, with or without emission
    print(f"{kind}: indirect ground truth, {int((a > b).sum())} channels brighter than direct-only, {int(nan.sum())} NaN")
    # how many pixels a bounce brightens is not predicted: several walls of the case world are wound outwards, and a bounce sampled about such a normal
    # leaves the room (the hit shaders do not turn normals towards the ray); that some pixel is brightened shows T * E at depth >= 1 arriving
    assert np.all((a >= b) | nan) and (a > b).any() and nan.mean() < 0.01, f"{kind}: the bounces add emission, never take any"
    gt1.close(); gu.close(); gw.close()
    gt.close(); gc.close(); g.close()


def ulp16_at_larger(a_bits, b_bits):
    a, b = a_bits.view(np.float16).astype(np.float64), b_bits.view(np.float16).astype(np.float64)
    big = np.maximum(np.abs(a), np.abs(b))
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(big, 2.0 ** -14))) - 10)
    return np.abs(a - b) / ulp


@pytest.mark.parametrize("kind,cutout", [("flat", False), ("private", False), ("shared", False), ("flat", True), ("shared", True)])
def test_additivity_on_a_lit_scene(hr, ctx, kind, cutout):
    """item 5: light on, first frame, infinite_bounces off; the device's emission-off image (pinned to the oracle by the existing suite) is the base.
    DDGI radiance with emission on is within 1 fp16 ulp (at the larger value) of fp16(float(off) + E): radiance is >= 0, so the base's rounding moves
    the sum by at most half an ulp of the result and the store adds half an ulp; two fp16 values less than two ulp apart are at most one apart.
    Reflections: the same against min(float(off) + E, 0.7) on traced texels where off < 0.7, both scenes' hit shaders gathering from the emission-free
    scene's DDGI atlases.  Textured emitters; cutout = True hides the cubes from
    every class (the GI class among them) through the alpha test."""
    W, H = ec.REFL_W, ec.REFL_H
    isd = ec.with_hidden_material(ec.instanced(), ec.CUBES) if cutout else ec.instanced()

    def scene(on):
        s = make(hr, ctx, isd, kind)
        if cutout:
            s.set_alpha_cutoffs(ec.cutoffs_for(ec.CUBES))
        return s.set_emission(True, 1.5).set_emissive_textures(ec.EMISSIVE_TEX) if on else s
    scenes = dict(off=scene(False), on=scene(True))

    # one pass set per scene; the reflections of BOTH scenes read the emission-free scene's DDGI atlases (with emission on the probes are lit by the
    # emitters too, which the trace kernel's own sum knows nothing of)
    import torch
    rig = rig_for(W, H)
    sets = dict(off=Passes(hr, ctx, rig, 1, ground_truth=False), on=Passes(hr, ctx, rig, 1, ground_truth=False))
    ubo = synth.make_ubo(ec.camera(W / H), None, ec.light())
    cur = ec.all_mirrors(gbuffer_np(scenes["off"], ubo, W, H))
    fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
    orient = synth_env.random_orientation(np.random.RandomState(4))
    fr = dict(ubo=ubo, cur=cur, orient=orient, f=0)
    snap = {}
    for tag in ("off", "on"):
        sets[tag].gi.params.infinite_bounces = 0
        sets[tag].gi.render(scenes[tag], fi, rig.env, orient)
        sets[tag].refl.ray_trace(scenes[tag], fi, rig.env, sets["off"].gi)
        torch.cuda.synchronize()
        snap[tag] = dict(ddgi_radiance=helpers.bits16(sets[tag].gi.image(sets[tag].gi.IMG_RADIANCE)), ddgi_direction_distance=helpers.bits16(sets[tag].gi.image(sets[tag].gi.IMG_DIRDIST)),
                         refl_trace=helpers.bits16(sets[tag].refl.image(sets[tag].refl.IMG_TRACE)))
    on, off = snap["on"], snap["off"]
    f16 = lambda b: b.view(np.float16).astype(F)
    # DDGI
    rays = ddgi_rays(rig, fr["orient"])
    E, prim = emission_of(scenes["on"], rays)
    assert np.array_equal(on["ddgi_direction_distance"], off["ddgi_direction_distance"]) and (E != 0).any(1).sum() > 20
    base = off["ddgi_radiance"].reshape(-1, 4)[:, :3]
    want = er.fp16_bits(f16(base) + E)
    d = ulp16_at_larger(on["ddgi_radiance"].reshape(-1, 4)[:, :3], want)
    print(f"{kind} cutout={cutout}: DDGI {int((E != 0).any(1).sum())} emitting rays, max distance {d.max():.2f} ulp, lit base texels {(base != 0).any(1).mean():.2f}")
    assert (base != 0).any(1).mean() > 0.3, "the base is lit"
    assert d.max() <= 1.0
    assert not np.array_equal(on["ddgi_radiance"], off["ddgi_radiance"])
    # reflections
    rays, traced = refl_rays(rig, sets["on"].refl, fr)
    E, prim = emission_of(scenes["on"], rays)
    E = E.reshape(H, W, 3)
    base = off["refl_trace"][..., :3]
    under = traced[..., None] & (f16(base) < F(0.7))
    want = er.fp16_bits(np.minimum(f16(base) + E, F(0.7)))
    d = ulp16_at_larger(on["refl_trace"][..., :3], want)
    print(f"{kind} cutout={cutout}: reflections {int(under.sum())} channels under the clamp of {int(traced.sum()) * 3}, max distance {d[under].max():.2f} ulp")
    assert under.mean() > 0.8 and (E[traced] != 0).any(-1).sum() > 20
    assert d[under].max() <= 1.0
    assert np.array_equal(on["refl_trace"][..., 3], off["refl_trace"][..., 3]), "the ray lengths do not change"
    for s in list(sets.values()) + list(scenes.values()):
        s.close()


def test_an_emitter_lights_the_room(hr, ctx):
    """item 6: the closed room, light intensity 0, a black sky, only the ceiling panel emits, DDGI with infinite bounces (128 rays per probe).  After
    two frames the irradiance atlas is non-zero for every probe with a clear line to the panel and all zero with emission off; a floor pixel of the
    composite (use_ddgi) is non-zero; after hr_deferred_add_emissive every texel is fp16(float(composite) + float(emissive image))"""
    import torch
    from hybrid_rendering_amd import api_deferred, api_gi
    W, H = 61, 37
    isd = ec.instanced(emissive=False)
    flat = isd.flatten()
    flat.tri_mesh_id = flat.tri_mesh_id.copy()
    flat.tri_mesh_id[:8] = 7                                    # the floor (the room's first wall) under a mesh id of its own
    rig = rig_for(W, H, black_sky=True, rays=128)
    ubo = synth.make_ubo(ec.camera(W / H), None, ec.light(0.0))
    atlas = {}
    for tag in ("on", "off"):
        g = hr.Scene(ctx, flat)
        if tag == "on":
            g.set_emission(True, 1.0).set_emissive(ec.panel_rgb())
        cur = gbuffer_np(g, ubo, W, H)
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
        gi = api_gi.DDGI(ctx, W, H, rig.ddgi)
        rng = np.random.RandomState(6)
        for f in range(2):
            gi.render(g, fi, rig.env, synth_env.random_orientation(rng))
        torch.cuda.synchronize()
        atlas[tag] = helpers.bits16(gi.current_read()[0])
        if tag == "on":
            # probes with a clear line to the panel: a ray to the centre of one of its four quads meets a panel triangle first
            first, _, _, n = isd.layout()
            panel = range(int(first[5]), int(first[5] + n[5]))
            u = rig.ddgi
            nx, ny, nz = (int(v) for v in u["probe_counts"])
            pos = np.array([[u["grid_start_position"][k] + u["grid_step"][k] * c[k] for k in range(3)] for c in
                            [(i % nx, (i % (nx * ny)) // nx, i // (nx * ny)) for i in range(nx * ny * nz)]], np.float64)
            clear = np.zeros(len(pos), bool)
            for centre in ((3, 9.95, 3), (7, 9.95, 3), (3, 9.95, 7), (7, 9.95, 7)):
                d = np.asarray(centre) - pos
                d /= np.linalg.norm(d, axis=1, keepdims=True)
                r = np.zeros((len(pos), 8), F)
                r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7] = pos, d, 1.0e4, 0.001
                prim = query(g, r)[0].cpu().numpy()
                clear |= np.isin(prim, panel)
            assert clear.sum() >= 20
            side = int(u["irradiance_probe_side_length"])
            lit = np.zeros(len(pos), bool)
            for i in range(len(pos)):
                col, row = i % (nx * ny), i // (nx * ny)
                cell = atlas["on"][row * (side + 2) + 2:row * (side + 2) + 2 + side, col * (side + 2) + 2:col * (side + 2) + 2 + side, :3]
                lit[i] = (cell.view(np.float16) > 0).any()
            assert lit[clear].all(), f"probes with a clear line to the panel and a dark atlas cell: {np.flatnonzero(clear & ~lit)}"
            # the composite, then the add stage
            df = api_deferred.DeferredShading(ctx, W, H)
            df.params.use_ray_traced_shadows = df.params.use_ray_traced_ao = df.params.use_ray_traced_reflections = 0
            df.render(fi, rig.env, gi=gi.output())
            torch.cuda.synchronize()
            before = helpers.bits16(df.output()).copy()
            ids = cur["gb3"][..., 2].view(np.float16).astype(np.int32)
            assert (ids == 7).sum() > 50 and (before[ids == 7][:, :3].view(np.float16) > 0).any(), "a floor pixel of the composite is lit by the panel alone"
            image = g.emissive_image(ubo, W, H)
            df.add_emissive(image)
            torch.cuda.synchronize()
            after, e = helpers.bits16(df.output()), helpers.bits16(image)
            f16 = lambda b: b.view(np.float16).astype(F)
            assert np.array_equal(after[..., :3], er.fp16_bits(f16(before[..., :3]) + f16(e[..., :3]))) and np.array_equal(after[..., 3], before[..., 3])
            on_panel = ids == 6
            assert on_panel.sum() > 20 and np.all(f16(e[on_panel][:, :3]) == F(4.0)) and not np.array_equal(after[on_panel], before[on_panel])
            # a wrong extent is refused
            with pytest.raises(hr.HRError, match="HR_ERR_INVALID_ARG"):
                df.add_emissive(torch.zeros((H, W + 1, 4), dtype=torch.float16, device="cuda"))
            df.close()
        gi.close(); g.close()
    assert not atlas["off"].view(np.float16)[..., :3].any(), "with emission off the room stays black"


def test_instrumented_traces_refuse_live_emission(hr, ctx):
    """item 7: hr_ddgi_trace_stats and hr_reflections_trace_stats return HR_ERR_UNSUPPORTED on a scene whose emission is live, leave the passes
    untouched, and run as ever once emission is disabled (or nothing emits)"""
    import torch
    W, H = ec.REFL_W, ec.REFL_H
    isd = ec.instanced()
    g = hr.Scene(ctx, isd.flatten()).set_emission(True, 1.0)
    rig = rig_for(W, H)
    ubo = synth.make_ubo(ec.camera(W / H), None, ec.light())
    cur = ec.all_mirrors(gbuffer_np(g, ubo, W, H))
    fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(cur), ubo, 0)
    p = Passes(hr, ctx, rig, 1, ground_truth=False)
    before = p.render(g, fi, ubo, synth_env.random_orientation(np.random.RandomState(1)))
    calls = (lambda: p.gi.trace_stats(g, fi, rig.env), lambda: p.refl.trace_stats(g, fi, rig.env, p.gi))
    for stats in calls:
        with pytest.raises(hr.HRError, match="HR_ERR_UNSUPPORTED"):
            stats()
        assert "hr_scene_set_emission" in hr.lib().hr_last_error().decode()
    torch.cuda.synchronize()
    assert_equal_snapshots(p.snapshot(), before, "the refused calls enqueued nothing", keys=("ddgi_radiance", "ddgi_direction_distance", "refl_trace"))
    g.set_emission(False, 1.0)
    for stats in calls:
        assert stats()[0] > 0
    g.set_emission(True, 1.0).set_emissive(np.zeros((ec.N_MATERIALS, 3), F))
    for stats in calls:
        assert stats()[0] > 0, "enabled, and nothing emits"
    torch.cuda.synchronize()
    p.close(); g.close()


@pytest.mark.parametrize("kind", ["flat", "shared"])
def test_hybrid_frame_modes_agree_on_a_live_emission_scene(hr, ctx, kind):
    """hr_hybrid_frame_render over a scene whose emission is live, in serial, streams and graph mode, against the four render() calls: DDGI ray images
    and atlases, the reflections trace image and a-trous output, AO and shadows bit for bit, 4 frames with temporal feedback at 64 x 40.  Emission is
    switched off for frame 2 and on again for frame 3: the graph mode captures the 4-argument emissive launches, then the plain kernels, then the
    emissive ones again (hipGraphExecUpdate meets another kernel function; where it declines, the frame instantiates anew).  The frame has no
    composite, so hr_deferred_add_emissive is not its business (DESIGN.md §7 "Emissive materials")."""
    import torch
    from hybrid_rendering_amd import api_frame
    W, H = ec.REFL_W, ec.REFL_H
    isd = ec.instanced()
    rig = rig_for(W, H)
    modes = dict(calls=None, serial=api_frame.FRAME_SERIAL, streams=api_frame.FRAME_STREAMS, graph=api_frame.FRAME_GRAPH)
    scenes = {tag: make(hr, ctx, isd, kind).set_emission(True, 1.5).set_emissive_textures(ec.EMISSIVE_TEX) for tag in modes}
    dark = make(hr, ctx, isd, kind)
    sets = {tag: Passes(hr, ctx, rig, 1, ground_truth=False) for tag in list(modes) + ["dark"]}
    for p in sets.values():
        p.gi.params.infinite_bounces = 0      # the probe rays' radiance then holds no history: with emission off it is the never-emitting scene's
    shadows = {tag: hr.RayTracedShadows(ctx, W, H) for tag in sets}
    native = {tag: api_frame.HybridFrame(ctx, shadows[tag], sets[tag].ao, sets[tag].gi, sets[tag].refl) for tag, mode in modes.items() if mode is not None}
    rng = np.random.RandomState(9)
    light = ec.light()
    prev = None
    for f in range(4):
        live = f != 2
        for s in scenes.values():
            s.set_emission(live, 1.5)
        ubo = synth.make_ubo(ec.camera(W / H), None, light)
        cur = ec.all_mirrors(gbuffer_np(dark, ubo, W, H))
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
                scene = dark if tag == "dark" else scenes[tag]
                shadows[tag].render(scene, fi)
                p.render(scene, fi, ubo, orient)
            torch.cuda.synchronize()
            snap[tag] = p.snapshot()
            snap[tag]["shadow_mask"] = shadows[tag].image(shadows[tag].IMG_MASK).cpu().numpy()
        for tag in ("serial", "streams", "graph"):
            assert_equal_snapshots(snap[tag], snap["calls"], f"{kind}, frame {f} (emission {'on' if live else 'off'}): {tag} mode against the render() calls")
        # the emitters are in the images while emission is on; the visibility passes never see them
        assert np.array_equal(snap["graph"]["ddgi_radiance"], snap["dark"]["ddgi_radiance"]) == (not live), f"frame {f}: DDGI radiance against the scene that never emitted"
        assert np.array_equal(snap["graph"]["ddgi_direction_distance"], snap["dark"]["ddgi_direction_distance"]) and np.array_equal(snap["graph"]["shadow_mask"], snap["dark"]["shadow_mask"])
        assert np.array_equal(snap["graph"]["ao_masks"], snap["dark"]["ao_masks"])
        prev = cur
    inst, upd = native["graph"].graph_stats()
    assert inst >= 1 and inst + upd == 4
    for n in native.values():
        n.close()
    for p in list(sets.values()) + list(shadows.values()) + list(scenes.values()) + [dark]:
        p.close()
