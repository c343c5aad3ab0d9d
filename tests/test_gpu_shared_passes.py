"""AO, DDGI, reflections, the ground truth and the hybrid frame on SHARED instanced scenes (hr_scene_enable_two_level_passes: csrc/traverse2.h
trace2 with an entry node, csrc/shading.h surface_at from a Hit2, the *_shared / <SHARED> trace kernels of ao / ddgi / reflections /
ground_truth.hip).  The contract is the one of tests/test_gpu_instances_shared.py: a triangle is hit iff the watertight test accepts its
world-space vertices and the hit shading runs the private-copy scene's operations, so every image is the private-copy scene's (and, in exact
mode, the oracle's) BIT FOR BIT.  No tolerance anywhere in this file.

There is no CPU-side companion (a tests/test_shared_passes_host.py checking that SceneShading::inst_shared is filled for shared scenes only):
scene_shading_from reads an hr_scene, and every way to make one — all the hr_scene_create* calls — needs a device, so the check is not
reachable without a GPU.  Here it is implied: a null inst_shared on a shared scene faults, a stale one on another kind is never read, and
test_the_switch_itself / test_one_identity_instance_is_the_flat_scene run the same pass objects on both kinds.  The two new symbols' declaration,
export and Python / C++ mirrors are checked without a GPU by tests/test_abi.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from hybrid_rendering_amd import synth, synth_env
from test_gpu_instances import _mats
from test_gpu_instances_shared import hostile_instances

pytestmark = pytest.mark.gpu

ROOM_LO, ROOM_HI = (0.0, 0.0, 0.0), (100.0, 100.0, 100.0)   # synth.instanced_cornell's room


class Rig:
    """blue-noise tables, environment and DDGI grid shared by every pass set of a test"""

    def __init__(self, W, H, lo, hi, probes=(3, 3, 3), rays=32, normal_bias=1.0):
        import torch
        from hybrid_rendering_amd import api_gi
        self.W, self.H = W, H
        self.sob, self.sr = synth.blue_noise_tables()
        self.sob_d, self.sr_d = torch.from_numpy(self.sob).cuda(), torch.from_numpy(self.sr).cuda()
        self.ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=probes, rays_per_probe=rays, normal_bias=normal_bias)
        self.sky = synth_env.sky_cubemap(16)
        self.pre, self.lut = synth_env.prefiltered_chain(self.sky, 5), synth_env.brdf_lut(16)
        self.env_np = dict(sky=self.sky, prefiltered=self.pre, pre_size=16, pre_levels=5, lut=self.lut)
        f16 = lambda a: torch.from_numpy(a).cuda().view(torch.float16)
        self.env = api_gi.environment(f16(self.sky), f16(self.pre), 16, 5, f16(self.lut))
        self.zbp = synth.z_buffer_params()

    def inputs(self, hr, cur_d, prev_d, ubo, f):
        return hr.frame_inputs(cur_d, prev_d, ubo, f, f & 1, self.sob_d, self.sr_d, z_buffer_params=self.zbp)


class Passes:
    """AO (2 spp, full resolution), DDGI, reflections (full resolution) and optionally the ground truth for ONE scene"""

    def __init__(self, hr, ctx, rig, exact=1, ground_truth=True):
        from hybrid_rendering_amd import api_gi, api_reflections, api_post
        self.hr, self.rig = hr, rig
        self.ao = hr.RayTracedAO(ctx, rig.W, rig.H, 0)
        self.ao.params.spp = 2
        self.gi = api_gi.DDGI(ctx, rig.W, rig.H, rig.ddgi)
        self.refl = api_reflections.RayTracedReflections(ctx, rig.W, rig.H, 0)
        self.gt = api_post.GroundTruthPathTracer(ctx, rig.W, rig.H) if ground_truth else None
        for p in (self.ao, self.gi, self.refl):
            p.params.exact = exact

    def render(self, scene, fi, ubo, orient):
        import torch
        self.ao.render(scene, fi)
        self.gi.render(scene, fi, self.rig.env, orient)
        self.refl.render(scene, fi, self.rig.env, self.gi)
        if self.gt is not None:
            self.gt.render(scene, ubo, self.rig.env)
        torch.cuda.synchronize()
        return self.snapshot()

    def snapshot(self):
        hr, mh = self.hr, (self.rig.H + 3) // 4
        irr, dep = self.gi.current_read()
        s = dict(ao_masks=self.ao.image(self.ao.IMG_MASK).cpu().numpy().view(np.uint32)[:2 * mh].copy(), ao_rays=self.ao.ray_count(),
                 ao_denoised=helpers.bits16(self.ao.output(hr.OUTPUT_ATROUS)),
                 ddgi_radiance=helpers.bits16(self.gi.image(self.gi.IMG_RADIANCE)), ddgi_direction_distance=helpers.bits16(self.gi.image(self.gi.IMG_DIRDIST)),
                 ddgi_irradiance=helpers.bits16(irr), ddgi_depth=helpers.bits16(dep),
                 refl_trace=helpers.bits16(self.refl.image(self.refl.IMG_TRACE)), refl_rays=self.refl.ray_count(),
                 refl_atrous=helpers.bits16(self.refl.output(hr.OUTPUT_ATROUS)))
        if self.gt is not None:
            s["ground_truth"] = helpers.bits16(self.gt.output())
        return s

    def close(self):
        for p in (self.ao, self.gi, self.refl, self.gt):
            if p is not None:
                p.close()


def assert_equal_snapshots(a, b, what, keys=None):
    for k in (keys or a.keys()):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs" + (f" on {int((np.asarray(a[k]) != np.asarray(b[k])).sum())} words" if np.shape(a[k]) else f" ({a[k]} vs {b[k]})")


def mirrors(cur):
    """gb3.x = 0.03 wherever the synthesiser wrote the default roughness 0.8: every surface pixel traces a mirror reflection ray"""
    ch = cur["gb3"][..., 0]
    ch[ch == np.float16(0.8).view(np.uint16)] = np.float16(0.03).view(np.uint16)
    return cur


def gbuffer_np(scene, ubo, W, H):
    """numpy G-buffer (uint16 bit patterns for the fp16 images, as the oracle's) synthesised on the GPU from `scene`"""
    out = {}
    for k, v in scene.gbuffer(ubo, W, H).items():
        a = v.cpu().numpy()
        out[k] = a.view(np.uint16) if a.dtype == np.float16 else a
    return out


def test_moving_instances_all_passes(oracle, hr, ctx):
    """instanced_cornell(9, seed 5), 160x120, 4 frames, every second instance moving, mirrors everywhere: AO 2 spp masks + ray count + denoised
    image, DDGI ray images + both atlases, reflections trace image + ray count + a-trous output and the ground truth of the opted-in shared scene
    against the private-copy scene (exact = 1 and exact = 0) and against oracle.InstancedScene (exact = 1); frames 1-3 run on the AO entry table
    rebuilt after update()"""
    from oracle import pyoracle_ddgi as od, pyoracle_reflections as orf, pyoracle_post as opost
    n_boxes, seed, W, H = 9, 5, 160, 120
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    g, gp, osc = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes(), hr.InstancedScene(ctx, isd), oracle.InstancedScene(isd)
    assert g.two_level_passes and not gp.two_level_passes
    lo, hi = isd.flatten().bounds()
    rig = Rig(W, H, lo, hi, probes=(4, 3, 4), rays=64)
    sets = {(tag, exact): Passes(hr, ctx, rig, exact) for tag in ("shared", "private") for exact in (1, 0)}
    oa = oracle.AOPass(W, H, spp=2, zbp=rig.zbp)
    odd, orr, ogt = od.DDGIPass(rig.ddgi), orf.ReflectionsPass(W, H), opost.GroundTruthPass(W, H)
    cams = helpers.cameras("cornell", W / H, 5, 1.0)
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(2)
    prev = None
    for f in range(4):
        mats = _mats(isd, n_boxes, seed, f)
        g.update(mats); gp.update(mats); osc.update(mats)
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = mirrors(osc.gbuffer(ubo, W, H))
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        snap = {k: p.render(g if k[0] == "shared" else gp, fi, ubo, orient) for k, p in sets.items()}
        for exact in (1, 0):
            assert_equal_snapshots(snap[("shared", exact)], snap[("private", exact)], f"frame {f}, exact = {exact}: shared against private copies")
        s = snap[("shared", 1)]
        assert s["ao_rays"] > 0 and s["refl_rays"] > 0
        oa.render(osc, ubo, cur, prev, rig.sob, rig.sr, f)
        mh = (H + 3) // 4
        assert np.array_equal(s["ao_masks"].reshape(2, mh, -1), oa.stages["mask"]), f"frame {f}: AO masks against the oracle"
        assert s["ao_rays"] == oa.stages["rays"] and np.array_equal(s["ao_denoised"], oa.stages["output"]), f"frame {f}: AO ray count / denoised image against the oracle"
        odd.render(osc, ubo, cur, rig.sky, orient, f)
        irr, dep = odd.current_read()
        assert np.array_equal(s["ddgi_radiance"], odd.stages["radiance"]), f"frame {f}: DDGI radiance against the oracle"
        assert np.array_equal(s["ddgi_direction_distance"], odd.stages["direction_distance"])
        assert np.array_equal(s["ddgi_irradiance"], irr) and np.array_equal(s["ddgi_depth"], dep), f"frame {f}: DDGI atlases against the oracle"
        orr.render(osc, ubo, rig.ddgi, cur, prev, rig.sob, rig.sr, f, rig.env_np, irr, dep, ping_pong=bool(f & 1))
        assert np.array_equal(s["refl_trace"], orr.stages["trace"]), f"frame {f}: reflections trace image against the oracle"
        assert s["refl_rays"] == orr.stages["rays"] and np.array_equal(s["refl_atrous"], orr.stages["atrous"][-1])
        assert np.array_equal(s["ground_truth"], ogt.render(osc, ubo, rig.sky)), f"frame {f}: ground truth against the oracle"
        prev = cur
    for p in list(sets.values()) + [g, gp]:
        p.close()


def _look_at(centre, radius, towards):
    """a camera 3 radii from `centre` on the side of `towards`, near / far planes scaled with the distance"""
    c, t = np.asarray(centre, np.float64), np.asarray(towards, np.float64)
    d = t - c
    d = d / np.linalg.norm(d) if np.linalg.norm(d) > 1e-3 * max(radius, 1e-30) else np.array([0.0, 0.3, 1.0]) / np.linalg.norm([0.0, 0.3, 1.0])
    dist = 3.0 * radius
    return synth.Camera(tuple(c + d * dist), tuple(c), fov=45.0, aspect=96 / 64, near=0.05 * dist, far=20.0 * dist)


def test_hostile_matrices(hr, ctx):
    """the matrix set of test_degenerate_and_hostile_matrices_against_the_flattened_scene (negative, zero, non-uniform, tiny and huge scales, a shear,
    ill-conditioned matrices on either side of the no_cull threshold), 96x64, one frame per camera: one camera per hostile instance that has any
    area, aimed at it from three of its radii away.  AO masks, DDGI radiance and the reflections trace image of the opted-in shared scene equal
    the private-copy scene's, and every one of those instances is what at least one traced pixel of its camera hits (the mesh id of the G-buffer
    synthesised from the shared scene).  The empty mesh and the instance collapsed to a point have no area: no ray can hit them in either scene."""
    W, H = 96, 64
    isd = hostile_instances(synth.instanced_cornell(4, seed=8))
    g, gp = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes(), hr.InstancedScene(ctx, isd)
    rig = Rig(W, H, ROOM_LO, ROOM_HI)
    ps, pp = Passes(hr, ctx, rig, 1, ground_truth=False), Passes(hr, ctx, rig, 1, ground_truth=False)
    flat = isd.flatten()
    first, _, _, n = isd.layout()
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(3)
    hostile = [(i, mid) for i, (_, _, mid) in enumerate(isd.instances) if mid >= 30 and mid not in (30, 32)]   # 30: the empty mesh, 32: the point
    assert len(hostile) == 10
    records = g.read_records()
    no_cull = {int(r[116:120].view(np.uint32)[0]) & 1 for r in records}
    assert no_cull == {0, 1}, "the set must hold an instance that is walked without object-space culling"
    for f, (i, mid) in enumerate(hostile):
        v = flat.verts[first[i]:first[i] + n[i]].reshape(-1, 3).astype(np.float64)
        centre, radius = 0.5 * (v.min(0) + v.max(0)), 0.5 * float(np.linalg.norm(v.max(0) - v.min(0)))
        ubo = synth.make_ubo(_look_at(centre, radius, (50.0, 50.0, 50.0)), None, light)
        cur = mirrors(gbuffer_np(g, ubo, W, H))
        ids = cur["gb3"][..., 2].view(np.float16)[cur["depth"] != 1.0]
        assert (ids == np.float16(mid)).any(), f"instance {i} (mesh id {mid}): no pixel of its camera hits it"
        cur_d = helpers.to_cuda(cur)
        fi = rig.inputs(hr, cur_d, cur_d, ubo, f)
        orient = synth_env.random_orientation(rng)
        a, b = ps.render(g, fi, ubo, orient), pp.render(gp, fi, ubo, orient)
        assert a["ao_rays"] > 0 and a["refl_rays"] > 0
        assert_equal_snapshots(a, b, f"camera on instance {i} (mesh id {mid})", keys=("ao_masks", "ao_rays", "ddgi_radiance", "ddgi_direction_distance", "refl_trace", "refl_rays"))
    for p in (ps, pp, g, gp):
        p.close()


def test_textured_instances_on_a_shared_scene(oracle, hr, ctx):
    """test_textured_instances on an opted-in shared scene: normal map (the (T, T, N) basis from the tangent transform_vertex rotated), roughness and
    metallic channels — DDGI radiance, reflections trace image and ground truth against the private copy and the oracle, two moving frames"""
    from oracle import pyoracle_ddgi as od, pyoracle_reflections as orf, pyoracle_post as opost
    n_boxes, seed, W, H = 7, 6, 128, 96
    isd = synth.instanced_cornell(n_boxes, seed=seed, textured=True)
    g, gp, osc = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes(), hr.InstancedScene(ctx, isd), oracle.InstancedScene(isd)
    lo, hi = isd.flatten().bounds()
    rig = Rig(W, H, lo, hi, rays=64)
    ps, pp = Passes(hr, ctx, rig, 1), Passes(hr, ctx, rig, 1)
    odd, orr, ogt = od.DDGIPass(rig.ddgi), orf.ReflectionsPass(W, H), opost.GroundTruthPass(W, H)
    cams = helpers.cameras("cornell", W / H, 3, 1.0)
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(4)
    prev = None
    for f in range(2):
        mats = _mats(isd, n_boxes, seed, f)
        g.update(mats); gp.update(mats); osc.update(mats)
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = mirrors(osc.gbuffer(ubo, W, H))
        prev = prev if prev is not None else cur
        fi = hr.frame_inputs(helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f, f & 1, rig.sob_d, rig.sr_d)
        orient = synth_env.random_orientation(rng)
        a, b = ps.render(g, fi, ubo, orient), pp.render(gp, fi, ubo, orient)
        assert_equal_snapshots(a, b, f"frame {f}: shared against private copies")
        odd.render(osc, ubo, cur, rig.sky, orient, f)
        assert np.array_equal(a["ddgi_radiance"], odd.stages["radiance"]), f"frame {f}: DDGI radiance against the oracle"
        irr, dep = odd.current_read()
        orr.render(osc, ubo, rig.ddgi, cur, prev, rig.sob, rig.sr, f, rig.env_np, irr, dep, ping_pong=bool(f & 1))
        assert np.array_equal(a["refl_trace"], orr.stages["trace"]), f"frame {f}: reflections trace image against the oracle"
        assert np.array_equal(a["ground_truth"], ogt.render(osc, ubo, rig.sky)), f"frame {f}: ground truth against the oracle"
        prev = cur
    for p in (ps, pp, g, gp):
        p.close()


def test_deforming_meshes(hr, ctx):
    """a shared=True, deformable=[...] scene: two synth.deform steps through update_meshes with a matrix update between them; after each step
    AO, DDGI, reflections and the ground truth equal those of a FRESH opted-in shared scene created over the same vertices and matrices, 96x64"""
    import torch
    import shared_deform_cases as sc
    W, H = 96, 64
    isd = sc.scene()
    g = hr.InstancedScene(ctx, isd, shared=True, deformable=sc.FLAGS).enable_two_level_passes()
    rig = Rig(W, H, ROOM_LO, ROOM_HI)
    ps, pf = Passes(hr, ctx, rig, 1), Passes(hr, ctx, rig, 1)
    cams = helpers.cameras("cornell", W / H, 3, 1.0)
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(6)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    mats = isd.matrices()
    for f, (kind, frame) in enumerate((("wave", 1), ("twist", 2))):
        d = synth.deform_meshes(isd, frame, kind, (sc.FIELD, sc.BOX))
        g.update_meshes([dict(mesh_idx=k, positions=cuda(d.meshes[k].verts), normals=cuda(d.meshes[k].normals)) for k in (sc.FIELD, sc.BOX)])
        if f == 1:
            mats = sc.moved(isd, 2)
            g.update(mats)          # the matrix update between the two mesh updates' renders
        fresh_isd = synth.InstancedSceneData(meshes=d.meshes, instances=[(m, k, mid) for m, (_, k, mid) in zip(mats, isd.instances)], materials=isd.materials)
        fresh = hr.InstancedScene(ctx, fresh_isd, shared=True).enable_two_level_passes()
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = mirrors(gbuffer_np(fresh, ubo, W, H))
        cur_d = helpers.to_cuda(cur)
        fi = rig.inputs(hr, cur_d, cur_d, ubo, f)
        orient = synth_env.random_orientation(rng)
        a, b = ps.render(g, fi, ubo, orient), pf.render(fresh, fi, ubo, orient)
        assert a["ao_rays"] > 0 and a["refl_rays"] > 0
        assert_equal_snapshots(a, b, f"step {f} ({kind}): updated scene against a fresh one")
        fresh.close()
    for p in (ps, pf, g):
        p.close()


def test_one_identity_instance_is_the_flat_scene(oracle, hr, ctx):
    """an opted-in shared scene with ONE identity instance against hr.Scene of the same triangles: AO, DDGI, reflections and ground truth, 3 frames"""
    sd = helpers.scene_data("sponza_small")
    one = synth.InstancedSceneData(meshes=[sd], instances=[(synth.model_matrix(), 0, 1)], materials=sd.materials)
    gi, gf = hr.InstancedScene(ctx, one, shared=True).enable_two_level_passes(), hr.Scene(ctx, sd)
    W, H = 256, 144
    frames = helpers.make_frames(oracle, oracle.Scene(sd), "sponza_small", W, H, 3, 1.0)
    lo, hi = sd.bounds()
    rig = Rig(W, H, lo, hi, probes=(5, 3, 4), rays=64, normal_bias=0.1)
    pi, pf = Passes(hr, ctx, rig, 1), Passes(hr, ctx, rig, 1)
    rng = np.random.RandomState(5)
    for f in range(3):
        cur, prev = frames[f]["gb"], frames[f - 1 if f else 0]["gb"]
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), frames[f]["ubo"], f)
        orient = synth_env.random_orientation(rng)
        a, b = pi.render(gi, fi, frames[f]["ubo"], orient), pf.render(gf, fi, frames[f]["ubo"], orient)
        assert a["ao_rays"] > 0 and a["refl_rays"] > 0
        assert_equal_snapshots(a, b, f"frame {f}: one identity instance against the flat scene")
    for p in (pi, pf, gi, gf):
        p.close()


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (65, 33)])
def test_ragged_and_tiny_images(hr, ctx, W, H):
    """1x1, 7x5 and 65x33: AO and reflections of the opted-in shared scene equal the private copy's — tiles whose edge lanes have no pixel, and (1x1:
    the camera's centre pixel alone) waves with hardly any ray at all"""
    isd = synth.instanced_cornell(4, seed=5)
    g, gp = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes(), hr.InstancedScene(ctx, isd)
    rig = Rig(W, H, ROOM_LO, ROOM_HI)
    ps, pp = Passes(hr, ctx, rig, 1, ground_truth=False), Passes(hr, ctx, rig, 1, ground_truth=False)
    cams = helpers.cameras("cornell", max(W / H, 1.0), 2, 1.0)
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(8)
    prev = None
    for f in range(2):
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = mirrors(gbuffer_np(gp, ubo, W, H))
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        a, b = ps.render(g, fi, ubo, orient), pp.render(gp, fi, ubo, orient)
        assert a["ao_rays"] > 0 and a["refl_rays"] > 0
        assert_equal_snapshots(a, b, f"{W}x{H}, frame {f}")
        prev = cur
    for p in (ps, pp, g, gp):
        p.close()


def test_shadows_and_ao_on_ragged_and_banded_images(hr, ctx):
    """65x33, the room and two instances, 2 frames (the second on the sorted launch list), shadows and AO (2 spp) as a whole frame and as the
    row band [16, 33) + halo 8 (resident rows from y0 = 8, launched in image order: a band has no launch list): the trace stage's mask words,
    per-tile ray slots and ray counts of the opted-in shared scene equal the private-copy scene's word for word.  The edge lanes of the ragged
    tiles read depth 0 and start on the camera's near plane, which lies outside the scene's box: the AO entry table misses and the descent runs
    (asserted from the geometry below, not observed in the kernel).  AO's per-tile ray slots have no accessor in the API: they are compared through
    their sum, hr_ao_ray_count, which for a band adds the zeros the untouched tiles were allocated with."""
    import torch
    W, H = 65, 33
    band = (16, 33, 8, 8)
    y0 = band[0] - band[2]
    isd = synth.instanced_cornell(2, seed=5)
    g, gp = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes(), hr.InstancedScene(ctx, isd)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    cams = helpers.cameras("cornell", W / H, 2, 1.0)
    light = helpers.light_for("cornell", "soft")

    def passes():
        p = dict(sh=hr.RayTracedShadows(ctx, W, H), ao=hr.RayTracedAO(ctx, W, H, 0), sh_band=hr.RayTracedShadows(ctx, W, H, 0, band=band), ao_band=hr.RayTracedAO(ctx, W, H, 0, band=band))
        p["ao"].params.spp = p["ao_band"].params.spp = 2
        return p

    ps, pp = passes(), passes()
    mh = (H + 3) // 4
    prev = None
    for f in range(2):
        assert cams[f].eye[2] - 2.0 * cams[f].near - ps["ao"].params.bias > max(g.info.bounds_hi[2], gp.info.bounds_hi[2]), "the near plane must lie outside the entry table's box"
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = gp.gbuffer(ubo, W, H)
        prev = prev if prev is not None else cur
        fi = hr.frame_inputs(cur, prev, ubo, f, f & 1, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
        snap = []
        for scene, p in ((g, ps), (gp, pp)):
            p["sh"].render(scene, fi); p["ao"].render(scene, fi)
            p["sh_band"].ray_trace(scene, fi); p["ao_band"].ray_trace(scene, fi)
            torch.cuda.synchronize()
            words = lambda q, planes: q.image(q.IMG_MASK).cpu().numpy().view(np.uint32)[:planes * mh].reshape(planes, mh, -1)
            snap.append(dict(shadow_mask=words(p["sh"], 1), shadow_slots=p["sh"].tile_ray_counts(), shadow_rays=p["sh"].ray_count(),
                             ao_masks=words(p["ao"], 2), ao_rays=p["ao"].ray_count(),
                             band_shadow_mask=words(p["sh_band"], 1)[:, y0 // 4:], band_shadow_slots=p["sh_band"].tile_ray_counts()[y0 // 8:],
                             band_shadow_rays=p["sh_band"].ray_count(), band_ao_masks=words(p["ao_band"], 2)[:, y0 // 4:], band_ao_rays=p["ao_band"].ray_count()))
        a, b = snap
        assert a["shadow_rays"] > 0 and a["ao_rays"] > 0 and a["band_shadow_rays"] == a["band_shadow_slots"].sum() > 0 and 0 < a["band_ao_rays"] < a["ao_rays"]
        assert_equal_snapshots(a, b, f"65x33, frame {f}")
        assert np.array_equal(a["band_shadow_mask"], a["shadow_mask"][:, y0 // 4:]) and np.array_equal(a["band_ao_masks"], a["ao_masks"][:, y0 // 4:]), f"frame {f}: the band's rows of the whole frame"
        prev = cur
    for p in list(ps.values()) + list(pp.values()) + [g, gp]:
        p.close()


def test_hybrid_frame_modes(hr, ctx):
    """hr_hybrid_frame_render in serial, streams and graph mode on the opted-in shared scene, 96x64, 2 frames: every output equals the four
    serial render() calls on the same scene"""
    import torch
    from hybrid_rendering_amd import api_frame
    W, H = 96, 64
    isd = synth.instanced_cornell(4, seed=5)
    g = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()
    rig = Rig(W, H, ROOM_LO, ROOM_HI)
    cams = helpers.cameras("cornell", W / H, 3, 1.0)
    light = helpers.light_for("cornell", "soft")
    modes = dict(calls=None, serial=api_frame.FRAME_SERIAL, streams=api_frame.FRAME_STREAMS, graph=api_frame.FRAME_GRAPH)
    sets, shadows, native = {}, {}, {}
    for tag, mode in modes.items():
        sets[tag], shadows[tag] = Passes(hr, ctx, rig, 1, ground_truth=False), hr.RayTracedShadows(ctx, W, H)
        if mode is not None:
            native[tag] = api_frame.HybridFrame(ctx, shadows[tag], sets[tag].ao, sets[tag].gi, sets[tag].refl)
    rng = np.random.RandomState(9)
    prev = None
    for f in range(2):
        g.update(_mats(isd, 4, 5, f))
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = mirrors(gbuffer_np(g, ubo, W, H))
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        snap = {}
        for tag, mode in modes.items():
            p = sets[tag]
            if mode is None:
                shadows[tag].render(g, fi)
                p.render(g, fi, ubo, orient)
            else:
                p.gi.set_orientation(orient)
                native[tag].render(g, rig.env, fi, fi, fi, fi, mode=mode)
            torch.cuda.synchronize()
            snap[tag] = p.snapshot()
            snap[tag]["shadow_mask"] = shadows[tag].image(shadows[tag].IMG_MASK).cpu().numpy()
            snap[tag]["shadows_denoised"] = helpers.bits16(shadows[tag].output(hr.OUTPUT_ATROUS))
            snap[tag]["ddgi_sample"] = helpers.bits16(p.gi.image(p.gi.IMG_SAMPLE))
        assert snap["calls"]["ao_rays"] > 0 and snap["calls"]["refl_rays"] > 0
        for tag in ("serial", "streams", "graph"):
            assert_equal_snapshots(snap[tag], snap["calls"], f"frame {f}: hybrid frame ({tag}) against the four render() calls")
        prev = cur
    for n in native.values():
        n.close()
    for p in list(sets.values()) + list(shadows.values()) + [g]:
        p.close()


def test_the_switch_itself(hr, ctx):
    """enable on a flat or private-copy scene: HR_ERR_INVALID_ARG; hr_scene_two_level_passes reports the state; after enable(0) the four passes
    refuse with the message of an un-opted scene and launch nothing; queries, the G-buffer and the shadows pass are the same bits with the flag on and off"""
    import torch
    from hybrid_rendering_amd import api_gi, api_reflections, api_post
    L = hr.lib()
    W, H = 96, 64
    isd = synth.instanced_cornell(4, seed=5)
    flat, gp = hr.Scene(ctx, synth.cornell32()), hr.InstancedScene(ctx, isd)
    g, twin = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)   # twin: never opted in
    for other in (flat, gp):
        assert L.hr_scene_enable_two_level_passes(other.h, C.c_int32(1)) == 1 and b"shared" in L.hr_last_error()   # HR_ERR_INVALID_ARG
        assert L.hr_scene_two_level_passes(other.h) == 0
    assert L.hr_scene_enable_two_level_passes(None, C.c_int32(1)) == 1 and L.hr_scene_two_level_passes(None) == 0
    assert L.hr_scene_two_level_passes(g.h) == 0, "off by default"
    rig = Rig(W, H, ROOM_LO, ROOM_HI)
    ubo = synth.make_ubo(helpers.cameras("cornell", W / H, 1, 0.0)[0], None, helpers.light_for("cornell", "soft"))
    rays = np.zeros((20000, 8), np.float32)
    rs = np.random.RandomState(3)
    rays[:, :3], d = rs.uniform(5, 95, (20000, 3)), rs.normal(size=(20000, 3))
    rays[:, 4:7], rays[:, 3], rays[:, 7] = d / np.linalg.norm(d, axis=1, keepdims=True), 1e4, 0.01
    rd = torch.from_numpy(rays).cuda()

    def untouched_by_the_flag(scene, shadows):
        cur = scene.gbuffer(ubo, W, H)
        fi = rig.inputs(hr, cur, cur, ubo, 0)
        shadows.reset_history()
        shadows.render(scene, fi)
        torch.cuda.synchronize()
        tuv, prim = scene.closest_hit(rd)
        out = [scene.any_hit(rd).cpu().numpy(), tuv.cpu().numpy().view(np.uint32), prim.cpu().numpy(), shadows.image(shadows.IMG_MASK).cpu().numpy(), helpers.bits16(shadows.output(hr.OUTPUT_ATROUS))]
        return out + [cur[k].cpu().numpy().view(np.uint8) for k in sorted(cur)], fi

    sh = hr.RayTracedShadows(ctx, W, H)
    off, fi = untouched_by_the_flag(g, sh)
    records_off = g.read_records()
    g.enable_two_level_passes()
    g.enable_two_level_passes()                                   # idempotent
    assert L.hr_scene_two_level_passes(g.h) == 1 and L.hr_scene_is_shared(g.h) == 1
    on, _ = untouched_by_the_flag(g, sh)
    assert all(np.array_equal(a, b) for a, b in zip(off, on)), "queries, G-buffer and shadows must not depend on the flag"
    assert np.array_equal(records_off, g.read_records())
    ps = Passes(hr, ctx, rig, 1)
    orient = synth_env.random_orientation(np.random.RandomState(1))
    cur = mirrors(gbuffer_np(g, ubo, W, H))
    cur_d = helpers.to_cuda(cur)
    fi = rig.inputs(hr, cur_d, cur_d, ubo, 0)
    first = ps.render(g, fi, ubo, orient)
    assert first["ao_rays"] > 0 and first["refl_rays"] > 0
    # statistics builds are refused on the opted-in scene, before anything is enqueued, in the shadows pass's words
    for call in (lambda: ps.ao.trace_stats(g, fi), lambda: ps.gi.trace_stats(g, fi, rig.env), lambda: ps.refl.trace_stats(g, fi, rig.env, ps.gi)):
        with pytest.raises(hr.HRError) as e:
            call()
        assert "HR_ERR_UNSUPPORTED" in str(e.value) and "trace statistics and developer switches are not available on a shared instanced scene" in str(e.value)
    g.enable_two_level_passes(False)
    assert L.hr_scene_two_level_passes(g.h) == 0
    calls = {"hr_ao_render": lambda s: ps.ao.render(s, fi), "hr_ddgi_render": lambda s: ps.gi.render(s, fi, rig.env, orient),
             "hr_reflections_render": lambda s: ps.refl.render(s, fi, rig.env, ps.gi), "hr_ground_truth_render": lambda s: ps.gt.render(s, ubo, rig.env)}
    images = {"hr_ao_render": lambda: ps.ao.image(ps.ao.IMG_MASK), "hr_ddgi_render": lambda: ps.gi.image(ps.gi.IMG_RADIANCE),
              "hr_reflections_render": lambda: ps.refl.image(ps.refl.IMG_TRACE), "hr_ground_truth_render": lambda: ps.gt.output()}
    bits = lambda t: t.contiguous().view(torch.uint8).clone()
    torch.cuda.synchronize()
    before = {name: bits(img()) for name, img in images.items()}
    for name, call in calls.items():
        messages = []
        for scene in (g, twin):
            with pytest.raises(hr.HRError) as e:
                call(scene)
            messages.append(str(e.value))
        assert messages[0] == messages[1], "after enable(0) the refusal reads as on a scene that never opted in"
        assert "HR_ERR_UNSUPPORTED" in messages[0] and name in messages[0] and "shared" in messages[0]
    torch.cuda.synchronize()
    for name, img in images.items():
        assert torch.equal(before[name], bits(img())), f"{name}: nothing may be launched once the flag is off again"
    for p in (ps, sh, g, twin, gp, flat):
        p.close()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERLANE_LIB = os.path.join(ROOT, "hybrid_rendering_amd", "variants", "libhybrid_rendering_amd.perlane2.so")


def test_cooperative_against_per_lane(hr, ctx, tmp_path):
    """trace_coop2 (the product library: the wave-cooperative triangle test on two levels, the default of AO, DDGI and reflections) against trace2,
    one ray per lane (the library built once more with -DAO_COOP2=0 -DDDGI_COOP2=0 -DREFL_COOP2=0 by __graft_entry__.build()): on the first two
    frames of test_moving_instances_all_passes, and on a 7x5 image whose tile has edge lanes that only serve as job lanes, the AO masks and the
    DDGI and reflections trace images are the same bits.  The test runs twice: here, and in a child process on the per-lane library, which only
    writes its images down."""
    n_boxes, seed = 9, 5
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    g = hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes()
    lo, hi = isd.flatten().bounds()
    light = helpers.light_for("cornell", "soft")
    mine = {}
    for W, H in ((160, 120), (7, 5)):
        rig = Rig(W, H, lo, hi, probes=(4, 3, 4), rays=64)
        ps = Passes(hr, ctx, rig, 1, ground_truth=False)
        cams = helpers.cameras("cornell", W / H, 3, 1.0)
        rng = np.random.RandomState(2)
        prev = None
        for f in range(2):
            g.update(_mats(isd, n_boxes, seed, f))
            ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
            cur = mirrors(gbuffer_np(g, ubo, W, H))
            prev = prev if prev is not None else cur
            fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
            s = ps.render(g, fi, ubo, synth_env.random_orientation(rng))
            assert s["ao_rays"] > 0 and s["refl_rays"] > 0
            for k in ("ao_masks", "ddgi_radiance", "ddgi_direction_distance", "refl_trace"):
                mine[f"{W}x{H}_{f}_{k}"] = s[k]
            prev = cur
        ps.close()
    g.close()
    dump = os.environ.get("HR_SHARED_PASSES_DUMP")
    if dump:                                   # the child process, on the per-lane library
        np.savez(dump, **mine)
        return
    assert os.path.exists(PERLANE_LIB), "build() makes hybrid_rendering_amd/variants/libhybrid_rendering_amd.perlane2.so"
    out_file = str(tmp_path / "perlane.npz")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_cooperative_against_per_lane", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, env=dict(os.environ, HR_LIBRARY=PERLANE_LIB, HR_SHARED_PASSES_DUMP=out_file), cwd=ROOT, timeout=600)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
    other = np.load(out_file)
    assert sorted(other.files) == sorted(mine)
    for k, v in mine.items():
        assert np.array_equal(v, other[k]), f"{k}: the cooperative and the per-lane two-level walk disagree"
