"""The two CLOSEST-HIT trace launches, k_ddgi_trace and k_refl_trace (flat, SHARED and CUTOUT instantiations, and the statistics builds), against
the oracle's passes run with BRUTE FORCE behind every query (orc_scene_set_brute_force: primary rays, the hit shader's light and sky rays) on
the crafted inputs of tests/closest_cases.py: rays exactly through vertices, shared edges, fan hubs and doubled triangles and 1 .. 8 ulps beside
them, hits at t_min / t_max +- ulps, probes in a triangle's plane and on the BVH's child-box planes, rays in face planes, all-miss and all-hit
probes, waves that straddle two probes, partial last waves, a one-ray-per-probe grid, an orientation that is no rotation, z-slab shards, the
first and a later frame (infinite bounces); reflections: the regime ties at roughness 0.05 / 0.75, tiles that are all sky / all rough / one
tracing lane / full / one rough lane among tracers and the converse, ragged tiles whose off-image lanes serve the cooperative walk, depth
beside 1 and above it, -0, bias 0, normals across and away from the camera, an over-long normal, GGX at trim 0 / 0.8 / 1 (each through misses
and through hits), misses exactly on the sky cube's seams (side / +Z and side / side) and a depth ulp beside them, hits whose 0.001 + t is
exactly an fp16 rounding tie of the stored ray_length, full and half resolution, and the same frame twice on one pass (the second launch runs in the cost order of the first).

Compared bit for bit, 0 mismatches: the reflections trace image (exact 1 and 0: it is bit-exact in both modes by contract) and ray_count();
the DDGI radiance and direction / distance images and ray_count().  tests/test_closest_cases.py pins the reference (the oracle's BVH pass
equals its brute-force pass on every case) and keeps these tests from passing vacuously.
Mutation results: docs/EXPERIMENTS.md, "Adversarial inputs for the closest-hit launches and the probe update"."""
import dataclasses

import numpy as np
import pytest

import closest_cases as cc
import helpers
from test_closest_cases import ddgi_reference, ddgi_references, refl_inputs, refl_reference, refl_references
from test_gpu_nonfinite import _put
from test_gpu_ray_edges import hexrow

pytestmark = pytest.mark.gpu


class Rig:
    def __init__(self, hr, ctx):
        import torch
        from hybrid_rendering_amd import api_gi, synth
        self.hr, self.ctx, self.torch, self.gi = hr, ctx, torch, api_gi
        sob, sr = synth.blue_noise_tables()
        self.sob, self.sr = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
        f16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().view(torch.float16)
        e = cc.coded_env()
        self.env = api_gi.environment(f16(e["sky"]), f16(e["prefiltered"]), e["pre_size"], e["pre_levels"], f16(e["lut"]))
        z = np.zeros((16, 16, 4), np.uint16)
        self.blank = helpers.to_cuda(dict(depth=np.zeros((16, 16), np.float32), gb2=z, gb3=z))

    # ---- DDGI
    def ddgi(self, case, gsc, stats=False):
        """(radiance, direction / distance, ray_count()[, trace_stats rays]) of ray_trace() on a fresh pass"""
        gp = self.gi.DDGI(self.ctx, 16, 16, case["ddgi"])
        try:
            gp.params.infinite_bounces, gp.params.infinite_bounce_intensity = int(case["infinite_bounces"]), 1.7
            gp.set_orientation(case["orientation"])
            if not case["first"]:
                gp.end_frame()
            irr, dep = cc.coded_atlases(case["ddgi"])
            ci, cd = gp.current_read()
            _put(ci, irr); _put(cd, dep)
            n, R = case["rays"].shape[:2]
            for which in (gp.IMG_RADIANCE, gp.IMG_DIRDIST):
                _put(gp.image(which), np.full((n, R, 4), cc.SENTINEL, np.uint16))
            if case["shard"] is not None:
                gp.set_shard(case["shard"][0], case["shard"][1], 0, 16)
            fi = self.hr.frame_inputs(self.blank, None, cc.plain_ubo(case["light"]), 0, 0, self.sob, self.sr)
            gp.ray_trace(gsc, fi, self.env)
            self.torch.cuda.synchronize()
            out = [helpers.bits16(gp.image(gp.IMG_RADIANCE)).reshape(n, R, 4), helpers.bits16(gp.image(gp.IMG_DIRDIST)).reshape(n, R, 4), int(gp.ray_count())]
            if stats:
                out.append(gp.trace_stats(gsc, fi, self.env)[0])
                self.torch.cuda.synchronize()
                out += [helpers.bits16(gp.image(gp.IMG_RADIANCE)).reshape(n, R, 4), helpers.bits16(gp.image(gp.IMG_DIRDIST)).reshape(n, R, 4)]
            return out
        finally:
            gp.close()

    # ---- reflections
    def reflections_pass(self, group, f, half_res=False):
        from hybrid_rendering_amd import api_reflections
        ddgi, irr, dep, _ = refl_inputs(group)
        g_ddgi = self.gi.DDGI(self.ctx, f["w"], f["h"], ddgi)
        ci, cd = g_ddgi.current_read()
        _put(ci, irr); _put(cd, dep)
        gp = api_reflections.RayTracedReflections(self.ctx, f["w"] * 2, f["h"] * 2, 1) if half_res else api_reflections.RayTracedReflections(self.ctx, f["w"], f["h"], 0)
        return gp, g_ddgi

    def reflections(self, gp, g_ddgi, gsc, f, exact=1):
        p = f["params"]
        for k in ("sample_gi", "approximate_with_ddgi", "gi_intensity", "rough_ddgi_intensity", "ibl_indirect_specular_intensity", "bias", "trim"):
            setattr(gp.params, k, p[k])
        gp.params.exact = exact
        cur = helpers.to_cuda(dict(depth=f["depth"], gb2=f["gb2"], gb3=f["gb3"]))
        fi = self.hr.frame_inputs(cur, cur, f["ubo"], 0, False, self.sob, self.sr, cur_full=cur)
        gp.ray_trace(gsc, fi, self.env, g_ddgi)
        self.torch.cuda.synchronize()
        return helpers.bits16(gp.image(gp.IMG_TRACE)).copy(), int(gp.ray_count()), fi


@pytest.fixture(scope="module")
def rig(hr, ctx):
    return Rig(hr, ctx)


def compare_ddgi(case, ref, got, what):
    rad, dd, count = got[:3]
    bad = np.argwhere((rad != ref["rad"]).any(-1) | (dd != ref["dd"]).any(-1))
    lines = []
    if len(bad):
        per = {}
        for p, r in bad:
            per[case.label(p, r)] = per.get(case.label(p, r), 0) + 1
        lines.append(f"  by family: {per}")
        for p, r in bad[:8]:
            lines.append(f"  (probe {p}, ray {r}) family {case.label(p, r)} ({int(case['ulps'][p, r]):+d}): radiance got {[hex(int(v)) for v in rad[p, r]]} want {[hex(int(v)) for v in ref['rad'][p, r]]}, "
                         f"direction / distance got {[hex(int(v)) for v in dd[p, r]]} want {[hex(int(v)) for v in ref['dd'][p, r]]}; brute-force winner {int(ref['prim'][p, r]) if 'prim' in ref else '?'}; "
                         f"ray o, t_max, d, t_min = {hexrow(case['rays'][p, r])}")
    if count != ref["count"]:
        lines.append(f"  ray_count() {count}, the reference traced {ref['count']}")
    print(f"{what}: {ref['count']} rays; {len(bad)} (probe, ray) texels differ")
    assert not lines, f"{what}: {len(bad)} (probe, ray) texels differ from the brute-force pass\n" + "\n".join(lines)


def compare_refl(f, ref, got, what):
    trace, count = got[:2]
    assert trace.shape == ref["trace"].shape, (what, trace.shape, ref["trace"].shape)
    bad = np.argwhere((trace != ref["trace"]).any(-1))
    lines = []
    if len(bad):
        per = {}
        for y, x in bad:
            per[f.label(y, x)] = per.get(f.label(y, x), 0) + 1
        lines.append(f"  by family: {per}")
        for y, x in bad[:8]:
            ray = ref["rays"][y, x]
            lines.append(f"  pixel ({x}, {y}) family {f.label(y, x)} ({int(f['ulps'][y, x]):+d}), regime {int(ray[3])}: got {[hex(int(v)) for v in trace[y, x]]} want {[hex(int(v)) for v in ref['trace'][y, x]]}; "
                         f"brute-force winner {int(ref['prim'][y, x])}; ray o, regime, d, traced = {hexrow(ray)}")
    if count != ref["count"]:
        lines.append(f"  ray_count() {count}, the reference traced {ref['count']}")
    print(f"{what}: {ref['count']} rays; {len(bad)} pixels differ")
    assert not lines, f"{what}: {len(bad)} pixels differ from the brute-force pass\n" + "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- flat scenes
def test_ddgi_trace_matches_the_brute_force_pass(oracle, hr, ctx, rig):
    """every DDGI case on hr.Scene: k_ddgi_trace<false, false>"""
    scenes = {}
    try:
        for case, osc, ref in ddgi_references():
            gsc = scenes.setdefault(id(case["sd"]), hr.Scene(ctx, case["sd"]))
            compare_ddgi(case, ref, rig.ddgi(case, gsc), f"ddgi/{case['name']}")
    finally:
        for s in scenes.values():
            s.close()


@pytest.mark.parametrize("exact", [1, 0])
def test_reflections_trace_matches_the_brute_force_pass(oracle, hr, ctx, rig, exact):
    """every reflections frame on hr.Scene, one pass object per group (its frames follow each other, the first one twice: the second launch
    runs in the cost order of the first), then the first frame at half resolution: k_refl_trace<false, false>"""
    for g, osc, frames in refl_references():
        gsc = hr.Scene(ctx, g["sd"])
        gp, g_ddgi = rig.reflections_pass(g, frames[0][0])
        hp, h_ddgi = rig.reflections_pass(g, frames[0][0], half_res=True)
        try:
            for i, (f, ref) in enumerate([frames[0]] + frames):
                compare_refl(f, ref, rig.reflections(gp, g_ddgi, gsc, f, exact), f"reflections/{g['name']}/{f['name']}/exact={exact}" + (" (first launch)" if i == 0 else ""))
            compare_refl(frames[0][0], frames[0][1], rig.reflections(hp, h_ddgi, gsc, frames[0][0], exact), f"reflections/{g['name']}/{frames[0][0]['name']}/half resolution/exact={exact}")
        finally:
            gp.close(); hp.close(); g_ddgi.close(); h_ddgi.close(); gsc.close()


# ---------------------------------------------------------------------------------------------------------------- statistics builds
def test_trace_stats_leave_the_images_and_count_the_reference_rays(oracle, hr, ctx, rig):
    """k_ddgi_trace<true> / k_refl_trace<true> (per-lane walks): the images are rewritten with the same bits, the ray count is the reference's"""
    case, osc, ref = [x for x in ddgi_references() if x[0]["name"] == "rot_r37"][0]
    gsc = hr.Scene(ctx, case["sd"])
    try:
        rad, dd, count, stat_rays, rad2, dd2 = rig.ddgi(case, gsc, stats=True)
        compare_ddgi(case, ref, (rad, dd, count), "ddgi/rot_r37 before trace_stats")
        compare_ddgi(case, ref, (rad2, dd2, stat_rays), "ddgi/rot_r37 after trace_stats, its ray count")
    finally:
        gsc.close()
    g, osc, frames = refl_references()[0]
    f, ref = frames[0]
    gsc = hr.Scene(ctx, g["sd"])
    gp, g_ddgi = rig.reflections_pass(g, f)
    try:
        trace, count, fi = rig.reflections(gp, g_ddgi, gsc, f)
        compare_refl(f, ref, (trace, count), "reflections/tiles before trace_stats")
        stat_rays = gp.trace_stats(gsc, fi, rig.env, g_ddgi)[0]
        rig.torch.cuda.synchronize()
        compare_refl(f, ref, (helpers.bits16(gp.image(gp.IMG_TRACE)), stat_rays), "reflections/tiles after trace_stats, its ray count")
    finally:
        gp.close(); g_ddgi.close(); gsc.close()


# ---------------------------------------------------------------------------------------------------------------- SHARED
def two_meshes(sd):
    """the scene as a shared instanced scene of two meshes under identity matrices, even triangles in one mesh and odd ones in the other: the two
    triangles of every tie pair (and the neighbours of every fan and shared edge) lie in different meshes"""
    from hybrid_rendering_amd import synth
    part = lambda s: synth.SceneData(np.ascontiguousarray(sd.verts[s]), np.ascontiguousarray(sd.normals[s]), np.ascontiguousarray(sd.tri_material[s]),
                                     np.ones(len(sd.verts[s]), np.uint32), sd.materials, "part")
    meshes = [part(slice(0, None, 2)), part(slice(1, None, 2))]
    return synth.InstancedSceneData(meshes=meshes, instances=[(synth.model_matrix(), 0, 1), (synth.model_matrix(), 1, 2)], materials=sd.materials, name=sd.name + "_two_level")


def test_two_level_kernels_match_the_brute_force_pass(oracle, hr, ctx, rig):
    """k_ddgi_trace<false, true> and k_refl_trace<false, true> on hr.InstancedScene(shared=True) with enable_two_level_passes(); the reference is
    the oracle's brute-force pass over the FLATTENED scene (mesh 0's triangles, then mesh 1's: the global triangle order the tie rule uses)"""
    for name in ("axis_3x2x2_r64", "rot_r37", "rot_r100"):
        case, _, _ = [x for x in ddgi_references() if x[0]["name"] == name][0]
        isd = two_meshes(case["sd"])
        osc = oracle.InstancedScene(isd)
        assert np.array_equal(np.sort(osc.verts.reshape(-1, 9).view(np.uint32), 0), np.sort(case["sd"].verts.reshape(-1, 9).view(np.uint32), 0)), "identity instances move a vertex"
        rad, dd, count = ddgi_reference(case, osc)
        gsc = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()
        try:
            compare_ddgi(case, dict(rad=rad, dd=dd, count=count), rig.ddgi(case, gsc), f"two-level ddgi/{name}")
        finally:
            gsc.close()
    for g, _, frames in refl_references():
        f, r = frames[0]
        isd = two_meshes(g["sd"])
        osc = oracle.InstancedScene(isd)
        trace, count = refl_reference(g, f, osc)
        gsc = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()
        gp, g_ddgi = rig.reflections_pass(g, f)
        try:
            compare_refl(f, dict(trace=trace, count=count, rays=r["rays"], prim=np.full(r["prim"].shape, -2)), rig.reflections(gp, g_ddgi, gsc, f), f"two-level reflections/{g['name']}/{f['name']}")
        finally:
            gp.close(); g_ddgi.close(); gsc.close()


# ---------------------------------------------------------------------------------------------------------------- CUTOUT
def textured(sd, alpha_of_material=None):
    """the scene with ONE 2x2 albedo texture on every material (white; alpha 255, or 0 in the texel at uv (0.75, 0.75)) and per-triangle constant
    uvs: (0.25, 0.25), or (0.75, 0.75) for the triangles whose material is in `alpha_of_material` (those hits are rejected by a cutoff of 0.5)"""
    tex = np.full((2, 2, 4), 255, np.uint8)
    uv = np.full((sd.n_tris, 3, 2), 0.25, np.float32)
    if alpha_of_material is not None:
        tex[1, 1, 3] = 0
        uv[np.isin(sd.tri_material, alpha_of_material)] = 0.75
    mt = np.full((len(sd.materials), 6), -1, np.int32)
    mt[:, 0] = 0
    mt[:, 4:6] = 0
    return dataclasses.replace(sd, uvs=uv, material_textures=mt, textures=[tex])


def test_cutout_kernels_with_an_all_opaque_alpha_table(oracle, hr, ctx, rig):
    """k_ddgi_trace<false, false, true> / k_refl_trace<false, false, true>: every material gets a cutoff of 0.5 over a texture whose alpha is 255
    everywhere, for the GI, reflection and shadow classes -> the brute-force pass over the same (textured) scene, bit for bit"""
    case, _, _ = [x for x in ddgi_references() if x[0]["name"] == "rot_r37"][0]
    sd = textured(case["sd"])
    osc = oracle.Scene(sd)
    rad, dd, count = ddgi_reference(case, osc)
    gsc = hr.Scene(ctx, sd).set_alpha_cutoffs(np.full(len(sd.materials), 0.5, np.float32))
    try:
        compare_ddgi(case, dict(rad=rad, dd=dd, count=count), rig.ddgi(case, gsc), "cutout (all opaque) ddgi/rot_r37")
    finally:
        gsc.close()
    g, _, frames = refl_references()[0]
    f, r = frames[0]
    sd = textured(g["sd"])
    osc = oracle.Scene(sd)
    trace, count = refl_reference(dict(g, sd=sd), f, osc)
    gsc = hr.Scene(ctx, sd).set_alpha_cutoffs(np.full(len(sd.materials), 0.5, np.float32))
    gp, g_ddgi = rig.reflections_pass(g, f)
    try:
        compare_refl(f, dict(trace=trace, count=count, rays=r["rays"], prim=np.full(r["prim"].shape, -2)), rig.reflections(gp, g_ddgi, gsc, f), "cutout (all opaque) reflections/tiles")
    finally:
        gp.close(); g_ddgi.close(); gsc.close()


def test_cutout_kernels_pass_a_rejected_texel_and_hit_what_lies_behind(oracle, hr, ctx, rig):
    """a checker alpha: the FIRST triangle of every doubled pair (rot_pair) maps to the texel whose alpha is 0 — its hit does not exist for the
    ray (class GI / reflection) nor for the light rays (class shadow), which go on to the identical triangle behind it.  The reference is the
    brute-force pass over the scene with those triangles collapsed to points (their indices stay)."""
    case, _, ref = [x for x in ddgi_references() if x[0]["name"] == "rot_r37"][0]
    first = np.unique(case["own"][case.of("rot_pair")][:, 0])
    assert len(first) > 40
    sd = textured(case["sd"], first)           # material i belongs to triangle i
    gone = dataclasses.replace(sd, verts=sd.verts.copy())
    gone.verts[first] = gone.verts[first][:, 0:1, :]
    osc = oracle.Scene(gone)
    rad, dd, count = ddgi_reference(case, osc)
    assert not np.array_equal(rad, ref["rad"]), "the rejected triangles change no bit"
    gsc = hr.Scene(ctx, sd).set_alpha_cutoffs(np.full(len(sd.materials), 0.5, np.float32))
    try:
        compare_ddgi(case, dict(rad=rad, dd=dd, count=count), rig.ddgi(case, gsc), "cutout (checker) ddgi/rot_r37")
    finally:
        gsc.close()
