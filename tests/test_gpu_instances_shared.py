"""Shared instanced scenes on the GPU (hr_scene_create_instanced_shared: one object-space BVH per mesh, walked on two levels —
csrc/instances_shared.hip, csrc/traverse2.h).  The contract: a triangle is hit iff the watertight test accepts its WORLD-space vertices, so
any-hit bytes, closest-hit records (t, u, v, global triangle), G-buffers and shadow images are the private-copy scene's and the flattened
scene's bit for bit; only the box culling runs in object space, widened by the per-(ray, instance) slack of DESIGN.md section 2.

Self-check of the slack (developer build, HR_CFLAGS=-DHR_SHARED_SLACK=0.0f, recorded in docs/EXPERIMENTS.md): with the slack forced to zero
test_edges_of_the_budget_against_brute_force must fail (measured: 1 of its 16 200 outside-origin edge rays picks another triangle)."""
import numpy as np
import pytest

import helpers
import ray_cases as rc
from hybrid_rendering_amd import synth
from test_gpu_instances import _mats, _rays
from test_instances_shared_host import heightfield

pytestmark = pytest.mark.gpu


def hexrow(r):
    return " ".join(float(x).hex() for x in r)


def answers(g, rd):
    occ = g.any_hit(rd).cpu().numpy()
    tuv, prim = [t.cpu().numpy() for t in g.closest_hit(rd)]
    return occ, tuv, prim


def assert_same(a, b, what):
    (occ, tuv, prim), (occ_b, tuv_b, prim_b) = a, b
    assert np.array_equal(occ, occ_b), f"{what}: any-hit differs on {int((occ != occ_b).sum())} rays"
    assert np.array_equal(prim, prim_b), f"{what}: closest-hit triangle differs on {int((prim != prim_b).sum())} rays"
    assert np.array_equal(tuv.view(np.uint32), tuv_b.view(np.uint32)), f"{what}: closest-hit t, u, v differ"


def compare_with_brute_force(gsc, osc, rays, what):
    """tests/test_gpu_ray_edges.py compare_with_brute_force: 0 mismatches against the oracle's brute force over the world-space triangles"""
    import torch
    ref_occ = osc.any_hit(rays, brute_force=True)
    ref_tuv, ref_prim = osc.closest_hit(rays, brute_force=True)
    occ, tuv, prim = answers(gsc, torch.from_numpy(np.ascontiguousarray(rays)).cuda())
    hit = ref_prim >= 0
    bad_any = (ref_occ != 0) != (occ != 0)
    bad_prim = ref_prim != prim
    bad_tuv = hit & (prim >= 0) & (ref_tuv.view(np.uint32) != tuv.view(np.uint32)).any(1)
    bad = bad_any | bad_prim | bad_tuv
    print(f"{what}: {len(rays)} rays, hit fraction {float((ref_occ != 0).mean()):.3f}; mismatches any-hit {int(bad_any.sum())}, primitive {int(bad_prim.sum())}, t/u/v {int(bad_tuv.sum())}")
    if bad.any():
        lines = [f"  ray {i}: {hexrow(rays[i])}\n    any-hit ref {int(ref_occ[i])} got {int(occ[i])}; closest ref prim {int(ref_prim[i])} t,u,v {hexrow(ref_tuv[i])}; got prim {int(prim[i])} t,u,v {hexrow(tuv[i])}"
                 for i in np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(rays)} rays differ from brute force (any-hit {int(bad_any.sum())}, primitive {int(bad_prim.sum())}, t/u/v {int(bad_tuv.sum())})\n" + "\n".join(lines))
    return int(bad.sum())


@pytest.mark.parametrize("n_boxes,seed", [(5, 3), (70, 9), (600, 4)])
def test_queries_after_every_update_equal_the_private_copy_and_the_flattened_scene(hr, ctx, n_boxes, seed):
    """the 6 / 71 / 601-instance configurations of tests/test_gpu_instances.py over the same updates, half the instances moving: 40 k rays, bit for bit"""
    import torch
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    g, gp = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd)
    assert hr.lib().hr_scene_is_shared(g.h) == 1 and hr.lib().hr_scene_is_shared(gp.h) == 0
    assert hr.lib().hr_scene_instance_count(g.h) == n_boxes + 1
    rd = torch.from_numpy(_rays(40000, seed)).cuda()
    for f in (0, 1, 2, 7, 90, 91):
        mats = _mats(isd, n_boxes, seed, f)
        g.update(mats)
        gp.update(mats)
        if f == 91:
            before = g.top_level_rebuilds
            g.rebuild_top_level()
            assert g.top_level_rebuilds == before + 1
        gf = hr.Scene(ctx, isd.flatten(mats))
        a = answers(g, rd)
        assert_same(a, answers(gp, rd), f"frame {f}: shared against private copies")
        assert_same(a, answers(gf, rd), f"frame {f}: shared against the flattened scene")
        info, finfo = g.refresh_info(), gf.info
        assert all(l <= fl for l, fl in zip(info.bounds_lo, finfo.bounds_lo)) and all(h >= fh for h, fh in zip(info.bounds_hi, finfo.bounds_hi)), "conservative bounds"
        gf.close()
        assert 0.05 < a[0].mean() < 0.999
    g.close(); gp.close()


ILL = ((2e-5, (40.0, 40.0, 55.0)), (2.2e-6, (60.0, 70.0, 25.0)), (1.8e-6, (25.0, 30.0, 75.0)))   # (second column's y, translation)


def hostile_instances(base):
    import dataclasses
    empty = dataclasses.replace(base.meshes[2], verts=np.zeros((0, 3, 3), np.float32), normals=np.zeros((0, 3, 3), np.float32), tri_material=np.zeros(0, np.uint32),
                                tri_mesh_id=np.zeros(0, np.uint32))
    meshes = list(base.meshes) + [empty]
    inst = list(base.instances)
    inst += [(synth.model_matrix((50, 50, 50)), 3, 30),                                   # the empty mesh
             (synth.model_matrix((30, 20, 60), (0, 1, 0), 0.4, (20, 0.0, 20)), 1, 31),    # squashed to a plane
             (synth.model_matrix((70, 20, 30), (1, 0, 0), 0.0, 0.0), 2, 32),              # a point
             (synth.model_matrix((4000, 3000, -2500), (1, 1, 0), 1.1, 15.0), 1, 33),      # far away
             (synth.model_matrix((60, 30, 40), (0, 0, 1), 0.7, (-12, 9, 14)), 2, 34),     # mirrored
             (synth.model_matrix((20, 60, 30), (1, 2, 3), 0.9, (25, 3, 11)), 1, 35),      # non-uniform
             (synth.model_matrix((45, 70, 70), (0, 1, 0), 0.3, 1e-4), 1, 36),             # tiny
             (synth.model_matrix((0, 0, 0), (0, 1, 1), 0.2, 1e4), 2, 37)]                 # huge: the whole room lies inside it
    shear = synth.model_matrix((75, 60, 20), (0, 0, 1), 0.0, 12.0).reshape(4, 4).copy()   # column-major rows = columns
    shear[1, 0] = 9.0; shear[2, 1] = -7.0                                                # column 1 leans along x, column 2 along y
    inst.append((shear.reshape(16), 1, 38))
    # two nearly parallel columns: condition number about 1e6, then one just below and one just above the 1e7 at which the builder stops
    # trusting the fp32 inverse and walks the instance without culling (instances_shared.hip fill_record: |A|_inf |A^-1|_inf)
    for (eps, at), mid in zip(ILL, (39, 40, 41)):
        ill = np.eye(4, dtype=np.float32)
        ill[0, :3] = (10.0, 0.0, 0.0); ill[1, :3] = (10.0, eps, 0.0); ill[2, :3] = (0.0, 0.0, 10.0); ill[3, :3] = at
        inst.append((ill.reshape(16), 2, mid))
    return synth.InstancedSceneData(meshes=meshes, instances=inst, materials=base.materials)


def test_degenerate_and_hostile_matrices_against_the_flattened_scene(hr, ctx):
    """the cases of test_degenerate_instances_against_the_flattened_scene (empty mesh, zero, negative scales, far away) plus non-uniform scales, a
    shear, scales of 1e-4 and 1e4, a matrix of condition number 1e6 and two on either side of the no-culling threshold (9e6 and 1.1e7 in the
    builder's measure): the shared scene equals the flattened one bit for bit, before and after updates"""
    import torch
    isd = hostile_instances(synth.instanced_cornell(4, seed=8))
    ill = [np.asarray(m, np.float32).astype(np.float64).reshape(4, 4).T[:3, :3] for m, _, _ in isd.instances[-3:]]
    assert 5e5 < np.linalg.cond(ill[0]) < 2e6
    measure = [np.abs(a).sum(1).max() * np.abs(np.linalg.inv(a)).sum(1).max() for a in ill]
    assert 5e5 < measure[0] < 2e6 and 8e6 < measure[1] < 1e7 < measure[2] < 1.3e7, measure
    g = hr.InstancedScene(ctx, isd, shared=True)
    rays = _rays(30000, 12)
    rng = np.random.RandomState(1)
    rays[:3000, :3] = np.array([3900, 2950, -2450], np.float32) + rng.uniform(-60, 60, (3000, 3)).astype(np.float32)   # around the far one
    rays[3000:5000, :3] = np.array([45, 70, 70], np.float32) + rng.uniform(-2e-4, 2e-4, (2000, 3)).astype(np.float32)   # around the tiny one
    for k, (_, at) in enumerate(ILL):                                                                                     # around the ill-conditioned ones
        rays[5000 + 1500 * k:6500 + 1500 * k, :3] = np.array(at, np.float32) + rng.uniform(-15, 15, (1500, 3)).astype(np.float32)
    rd = torch.from_numpy(rays).cuda()
    mats = isd.matrices()
    for step in range(3):
        if step:
            mats = mats.copy()
            mats[1:5, 12:15] += np.float32(3.5 * step)
            mats[8, 12:15] += np.float32(-500.0 * step)
            g.update(mats)
        gf = hr.Scene(ctx, isd.flatten(mats))
        a = answers(g, rd)
        assert_same(a, answers(gf, rd), f"step {step}")
        assert (a[2] >= 0).mean() > 0.5
        gf.close()
    g.close()


def edge_scene():
    """twelve rotated, non-uniformly scaled instances of the Cornell boxes' meshes (no room around them: rays from far away reach them)"""
    base = synth.instanced_cornell(3, seed=2)
    rng = np.random.RandomState(11)
    inst = []
    for i in range(12):
        axis = rng.normal(size=3)
        scale = tuple(float(s) for s in rng.uniform(0.3, 3.0, 3) * (10.0 if i % 2 else 1.0))
        t = tuple(float(x) for x in rng.uniform(-60, 60, 3))
        inst.append((synth.model_matrix(t, tuple(axis / np.linalg.norm(axis)), float(rng.uniform(0, 6.28)), scale), 1 + i % 2, 40 + i))
    return synth.InstancedSceneData(meshes=base.meshes, instances=inst, materials=base.materials)


def test_edges_of_the_budget_against_brute_force(oracle, hr, ctx):
    """rays through triangle edges and vertices, in the face planes of the meshes' leaf boxes (built in object space, sent through the instance's
    matrix) and of the instances' world boxes, from origins 1 to 1e6 scene diagonals away: every ray agrees with brute force over the world-space triangles"""
    isd = edge_scene()
    g = hr.InstancedScene(ctx, isd, shared=True)
    flat = isd.flatten()
    osc = oracle.Scene(flat)
    bad = 0
    try:
        bad += compare_with_brute_force(g, osc, rc.edge_and_vertex_rays(flat.verts, seed=1), "shared/edge_and_vertex")
        bad += compare_with_brute_force(g, osc, rc.edge_and_vertex_rays(flat.verts, seed=2, origins="outside"), "shared/edge_and_vertex from outside")
        for factors in ((1.0, 10.0), (1e2, 1e3), (1e4, 1e5), (1e6,)):
            bad += compare_with_brute_force(g, osc, rc.far_origin_rays(flat.verts, factors=factors, seed=3, max_tris=300), f"shared/far origins x{factors}")
        # the instances' world boxes
        first, _, _, n = isd.layout()
        boxes = np.stack([np.stack([flat.verts[f:f + k].reshape(-1, 3).min(0), flat.verts[f:f + k].reshape(-1, 3).max(0)]) for f, k in zip(first, n)]).astype(np.float32)
        bad += compare_with_brute_force(g, osc, rc.box_grazers(boxes, seed=4), "shared/instance box grazers")
        # leaf boxes of a mesh's object-space tree: grazing rays built in object space, carried to world space through each instance's matrix
        for i, (m, k, _) in enumerate(isd.instances[:6]):
            cb = hr.bvh_child_boxes(isd.meshes[k].verts)
            orays = rc.box_grazers(cb[cb["is_leaf"] != 0][:40], seed=5 + i)
            M = np.asarray(m, np.float64).reshape(4, 4).T          # column-major -> [row][column]
            w = orays.copy()
            w[:, 0:3] = (orays[:, 0:3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
            w[:, 4:7] = (orays[:, 4:7].astype(np.float64) @ M[:3, :3].T).astype(np.float32)    # not normalised: t keeps its meaning
            bad += compare_with_brute_force(g, osc, w, f"shared/leaf box grazers of instance {i}")
    finally:
        g.close()
    assert bad == 0


def test_shadows_pass_and_gbuffer_equal_the_private_copy_scene(oracle, hr, ctx):
    """the moving-instance sequence of test_passes_on_a_scene_whose_instances_move_every_frame, shadows only, 4 frames, both arithmetic modes:
    G-buffers, masks, tile classes and every stage image of the shared scene equal the private-copy scene's; exact mode: the oracle's too"""
    import torch
    n_boxes, seed, W, H = 9, 5, 160, 120
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    g, gp, osc = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd), oracle.InstancedScene(isd)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    cams = helpers.cameras("cornell", W / H, 5, 1.0)
    light = helpers.light_for("cornell", "soft")
    passes = {}
    for exact in (1, 0):
        a, b = hr.RayTracedShadows(ctx, W, H), hr.RayTracedShadows(ctx, W, H)
        a.params.exact = b.params.exact = exact
        passes[exact] = (a, b)
    os_ = oracle.ShadowsPass(W, H)
    prev_np = None
    for f in range(4):
        mats = _mats(isd, n_boxes, seed, f)
        g.update(mats); gp.update(mats); osc.update(mats)
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur_s, cur_p, cur = g.gbuffer(ubo, W, H), gp.gbuffer(ubo, W, H), osc.gbuffer(ubo, W, H)
        for k in cur:
            got = cur_s[k].cpu().numpy()
            assert np.array_equal(got, cur_p[k].cpu().numpy()), f"frame {f}: G-buffer {k}: shared against private copies"
            assert np.array_equal(got.view(np.uint16) if got.dtype == np.float16 else got, cur[k]), f"frame {f}: G-buffer {k} against the oracle"
        prev = prev_np if prev_np is not None else cur
        fi = hr.frame_inputs(helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f, f & 1, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
        os_.render(osc, ubo, cur, prev, sob, sr, f)
        for exact, (ps, pp) in passes.items():
            ps.render(g, fi); pp.render(gp, fi)
            torch.cuda.synchronize()
            for img in (ps.IMG_MASK, ps.IMG_TEMPORAL, ps.IMG_MOMENTS0, ps.IMG_MOMENTS1, ps.IMG_PREV, ps.IMG_ATROUS0, ps.IMG_ATROUS1, ps.IMG_UPSAMPLE, ps.IMG_TILES):
                x, y = ps.image(img).cpu().numpy(), pp.image(img).cpu().numpy()
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"frame {f}, exact = {exact}: image {img}"
            assert np.array_equal(helpers.bits16(ps.output(hr.OUTPUT_ATROUS)), helpers.bits16(pp.output(hr.OUTPUT_ATROUS)))
            assert ps.ray_count() == pp.ray_count()
            if exact:
                assert np.array_equal(ps.image(ps.IMG_MASK).cpu().numpy().view(np.uint32), os_.stages["mask"]), f"frame {f}: shadow mask against the oracle"
                assert np.array_equal(helpers.bits16(ps.output(hr.OUTPUT_ATROUS)), os_.stages["output"]), f"frame {f}: denoised shadows against the oracle"
        prev_np = cur
    for ps, pp in passes.values():
        ps.close(); pp.close()
    g.close(); gp.close()


def test_beyond_the_private_copy_limit(hr, ctx):
    """1024 instances of a 2^16-triangle mesh (2^26 references as private copies: refused) on a grid with gaps, as a shared scene; 20 000 ray
    segments, each confined to one instance's grid cell, answer as a one-instance PRIVATE-COPY scene holding that instance alone does (the single-level walk: an independent reference)"""
    import torch
    mesh = heightfield(128, 256)
    side, pitch = 32, 2.0
    rng = np.random.RandomState(7)
    inst = []
    for i in range(side * side):
        ang = float(rng.uniform(0, 6.28))
        inst.append((synth.model_matrix((pitch * (i % side) + 0.5, 0.0, pitch * (i // side) + 0.5), (0, 1, 0), ang, (0.7, 1.0 + (i % 3), 0.7)), 0, 1 + i))
    isd = synth.InstancedSceneData(meshes=[mesh], instances=inst, materials=mesh.materials)
    st, fp = hr.instanced_scene_footprint(isd, shared=False)
    assert st == 5
    st, fp = hr.instanced_scene_footprint(isd, shared=True)
    assert st == 0
    g = hr.InstancedScene(ctx, isd, shared=True)
    info = g.refresh_info()
    assert (info.n_tris, info.n_nodes, info.max_depth, int(info.node_bytes), int(info.tri_bytes)) == (fp.n_tris, fp.n_nodes, fp.max_depth, int(fp.node_bytes), int(fp.tri_bytes))
    assert list(info.bounds_lo) == list(fp.bounds_lo) and list(info.bounds_hi) == list(fp.bounds_hi)
    # a rotated 0.7 x 0.7 footprint around (0.5, 0.5) of its cell stays within radius 0.5 of the cell's centre + 0.5: inside the 2 x 2 cell
    n, n_cells = 20000, 40
    cells = rng.choice(side * side, n_cells, replace=False)
    cell = cells[rng.randint(0, n_cells, n)]
    c0 = np.stack([pitch * (cell % side), np.zeros(n), pitch * (cell // side)], 1) + np.array([-0.45, -0.5, -0.45])
    ext = np.array([1.9, 5.0, 1.9])
    p0, p1 = c0 + rng.uniform(0, 1, (n, 3)) * ext, c0 + rng.uniform(0, 1, (n, 3)) * ext
    # three of five segments run towards the middle of the instance's footprint (the mesh's centre through its matrix), so that most of them hit
    centre = np.stack([np.asarray(inst[c][0], np.float64).reshape(4, 4).T @ np.array([0.5, 0.0, 0.5, 1.0]) for c in cell])[:, :3]
    aimed = rng.uniform(size=n) < 0.6
    for a, (r0, r1) in ((0, (0.4, 0.2)), (2, (0.4, 0.2))):
        p0[aimed, a] = centre[aimed, a] + rng.uniform(-r0, r0, int(aimed.sum()))
        p1[aimed, a] = centre[aimed, a] + rng.uniform(-r1, r1, int(aimed.sum()))
    p0[:, 1] = rng.uniform(0.5, 4.5, n)                  # start above the surface, end below it
    p1[:, 1] = rng.uniform(-0.5, -0.3, n)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = p0, p1 - p0, 1.0, 0.0       # o + t d, t in (0, 1): the segment
    end = rays[:, 0:3] + rays[:, 4:7]
    assert (rays[:, 0:3] >= c0.astype(np.float32)).all() and (end <= (c0 + ext).astype(np.float32)).all()
    rd = torch.from_numpy(rays).cuda()
    occ, tuv, prim = answers(g, rd)
    assert (prim >= 0).mean() >= 0.25 and occ.mean() >= 0.25, "at least a quarter of the segments must hit"
    for c in cells:
        sel = np.flatnonzero(cell == c)
        one = hr.InstancedScene(ctx, synth.InstancedSceneData(meshes=[mesh], instances=[inst[c]], materials=mesh.materials))
        assert hr.lib().hr_scene_is_shared(one.h) == 0
        o1, t1, p1_ = answers(one, rd[torch.from_numpy(sel).cuda()])
        one.close()
        rebased = np.where(p1_ >= 0, p1_ + c * mesh.n_tris, -1)
        assert np.array_equal(occ[sel], o1) and np.array_equal(prim[sel], rebased) and np.array_equal(tuv[sel].view(np.uint32), t1.view(np.uint32)), f"cell {c}"
    g.close()


def test_unsupported_passes_refuse_a_shared_scene_and_still_render_others(hr, ctx):
    """AO, DDGI, reflections and the ground truth return HR_ERR_UNSUPPORTED for a shared scene, naming the pass, and launch nothing: their images
    stay as they were; the same pass objects render a private-copy scene afterwards"""
    import torch
    from hybrid_rendering_amd import api_gi, api_reflections, api_post, synth_env
    W, H = 96, 64
    isd = synth.instanced_cornell(4, seed=5)
    g, gp = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    lo, hi = isd.flatten().bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 3, 3), rays_per_probe=32, normal_bias=1.0)
    sky = synth_env.sky_cubemap(16)
    f16 = lambda a: torch.from_numpy(a).cuda().view(torch.float16)
    env = api_gi.environment(f16(sky), f16(synth_env.prefiltered_chain(sky, 5)), 16, 5, f16(synth_env.brdf_lut(16)))
    ubo = synth.make_ubo(helpers.cameras("cornell", W / H, 1, 0.0)[0], None, helpers.light_for("cornell", "soft"))
    cur = gp.gbuffer(ubo, W, H)
    cur["gb3"][..., 0] = 0.03                           # mirrors everywhere: the reflections pass traces a ray for every surface pixel
    fi = hr.frame_inputs(cur, cur, ubo, 0, 0, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
    ga, gd, gr = hr.RayTracedAO(ctx, W, H, 0), api_gi.DDGI(ctx, W, H, ddgi), api_reflections.RayTracedReflections(ctx, W, H, 0)
    gt = api_post.GroundTruthPathTracer(ctx, W, H)
    orient = synth_env.random_orientation(np.random.RandomState(1))
    calls = {"hr_ao_render": lambda s: ga.render(s, fi), "hr_ddgi_render": lambda s: gd.render(s, fi, env, orient),
             "hr_reflections_render": lambda s: gr.render(s, fi, env, gd), "hr_ground_truth_render": lambda s: gt.render(s, ubo, env)}
    images = {"hr_ao_render": lambda: ga.image(ga.IMG_MASK), "hr_ddgi_render": lambda: gd.image(gd.IMG_RADIANCE),
              "hr_reflections_render": lambda: gr.image(gr.IMG_TRACE), "hr_ground_truth_render": lambda: gt.output()}
    bits = lambda t: t.contiguous().view(torch.uint8).clone()
    before = {name: bits(img()) for name, img in images.items()}
    for name, call in calls.items():
        with pytest.raises(hr.HRError) as e:
            call(g)
        assert "HR_ERR_UNSUPPORTED" in str(e.value) and name in str(e.value) and "shared" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for name, img in images.items():
        assert torch.equal(before[name], bits(img())), f"{name}: nothing may be launched for a shared scene"
    for name, call in calls.items():
        call(gp)
    torch.cuda.synchronize()
    for name, img in images.items():
        assert int(bits(img()).ne(before[name]).sum()) > 0, f"{name}: the pass renders a private-copy scene afterwards"
    for p in (ga, gd, gr, gt, g, gp):
        p.close()


def test_axis_parallel_rays_with_tiny_directions_on_a_large_instance(oracle, hr, ctx):
    """the 1e-18 clamp of a zero direction component (traverse2.h boxray_object): one cube scaled by 1e4, rays exactly along an axis with
    |d| = 1e-12, so hits lie at t ~ 1e16 and the clamped components would carry the object-space ray 1e-2 object units sideways — half of the
    rays run within 2e-2 of the cube's edges, where that is enough to leave its boxes.  Against the flattened scene and brute force."""
    import torch
    base = synth.instanced_cornell(2, seed=1)
    cube = base.meshes[1]
    S = 1e4
    isd = synth.InstancedSceneData(meshes=[cube], instances=[(synth.model_matrix((0, 0, 0), (0, 1, 0), 0.0, S), 0, 1)], materials=base.materials)
    lo, hi = [b.astype(np.float64) for b in cube.bounds()]
    rng = np.random.RandomState(3)
    n = 6000
    rays = np.zeros((n, 8), np.float32)
    rays[:, 3], rays[:, 7] = 1e30, 0.0
    for i in range(n):
        ax = i % 3
        p = rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo))
        if i & 1:                                       # close to the edge the clamp (always +1e-18) drifts towards
            side = (ax + 1 + (i >> 1) % 2) % 3
            p[side] = hi[side] + rng.uniform(-0.02, 0.005) * (hi[side] - lo[side])
        sign = 1.0 if (i >> 2) & 1 else -1.0
        p[ax] = lo[ax] - (hi[ax] - lo[ax]) if sign > 0 else hi[ax] + (hi[ax] - lo[ax])
        rays[i, 0:3] = p * S
        rays[i, 4 + ax] = sign * 1e-12
    g, flat = hr.InstancedScene(ctx, isd, shared=True), isd.flatten()
    gf = hr.Scene(ctx, flat)
    rd = torch.from_numpy(rays).cuda()
    a = answers(g, rd)
    assert_same(a, answers(gf, rd), "axis-parallel rays: shared against the flattened scene")
    assert compare_with_brute_force(g, oracle.Scene(flat), rays, "shared/axis-parallel tiny directions") == 0
    assert 0.5 < (a[2] >= 0).mean() < 0.99
    g.close(); gf.close()


def test_an_update_rewrites_the_top_level_and_the_records_only(hr, ctx):
    """hr_scene_read_bvh before and after updates (a forced top-level re-build included): the meshes' nodes and every triangle reference read back
    identical — object space, never touched — while the top level's slots change"""
    n_boxes, seed = 70, 9
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    g = hr.InstancedScene(ctx, isd, shared=True)
    top = n_boxes + 1                                   # include/hr_api_stages.h: max(1, n_instances) top-level slots
    nodes0, tris0 = g.read_bvh()
    assert len(tris0) == sum(int(hr.bvh_build_info(m.verts).tri_bytes) // 48 for m in isd.meshes), "one set of references per MESH"
    for f in (1, 2, 90):
        g.update(_mats(isd, n_boxes, seed, f))
    g.rebuild_top_level()
    nodes1, tris1 = g.read_bvh()
    assert np.array_equal(tris0, tris1) and np.array_equal(nodes0[top:], nodes1[top:])
    assert not np.array_equal(nodes0[:top], nodes1[:top])
    g.close()
