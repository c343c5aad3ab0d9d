"""Hostile vertex streams (tests/deform_cases.py) through hr_scene_update_vertices and hr_scene_update_meshes: creation from a placeholder, inflation
and collapse by 2^+-30, drift to 2^20, non-finite vertices.  The contract of csrc/deform.hip needs no tolerance — "a query's answer is the one a
fresh build over the same vertices gives" — so ONE live scene walks each stream and after every step answers bit for bit like hr_scene_create over
that step's vertices and like the oracle's brute force; its boxes hold what they must (test_gpu_deformable.check_boxes, which counts non-finite
triangles for nothing, as the builder does); and a step back to the base leaves the node bytes of a scene that never saw the hostile steps.
That the streams can tell right from wrong is tests/test_deform_cases.py's business (oracle alone)."""
import numpy as np
import pytest

import deform_cases as dc
import helpers
import ray_cases as rc
from hybrid_rendering_amd import synth
from test_gpu_deformable import check_boxes, cuda, own_boxes
from test_gpu_instances_shared import answers, assert_same, compare_with_brute_force

pytestmark = pytest.mark.gpu
F32 = np.float32


def put(g, verts, first=0, count=None):
    count = len(verts) - first if count is None else count
    g.update_vertices(cuda(verts[first:first + count]), None, first_tri=first)


def a_leaf(g):
    """the triangles of the scene's fullest leaf"""
    boxes, leaf, nodes, tris = own_boxes(g)
    prim = tris.reshape(-1, 48)[:, 12:16].copy().view(np.uint32)[:, 0]
    rows = leaf[boxes["is_leaf"] == 1]
    first, count = rows[np.argmax(rows[:, 1])]
    assert count >= 2
    return [int(p) for p in prim[first:first + count]]


def check_answers(hr, ctx, oracle, g, sd0, st, what, seed, own=True):
    """every ray set of the step: the live scene against hr_scene_create over the step's vertices and against brute force, 0 mismatches"""
    from hybrid_rendering_amd import api
    sd = dc.with_verts(sd0, st.verts)
    finite, _ = dc.strip_nonfinite(st.verts)
    fresh = api.bvh_child_boxes(finite) if len(finite) else None
    sets = dc.ray_sets(st, fresh, own_boxes(g)[0] if own and len(finite) else None, seed=seed, base=sd0.verts)
    gf, osc = hr.Scene(ctx, sd), oracle.Scene(sd)
    for name, rays in sets.items():
        assert dc.sound(osc, st.verts, rays).all(), f"{what}/{name}: the reference hits by rounding alone"
        a = answers(g, cuda(rays))
        assert_same(a, answers(gf, cuda(rays)), f"{what}/{name}: refitted against a fresh scene")
        assert compare_with_brute_force(g, osc, rays, f"{what}/{name}") == 0
        if st.kind == "nothing":
            assert not a[0].any() and (a[2] < 0).all(), f"{what}/{name}: a hit where nothing can be hit"
    gf.close()


def check_rebuild(hr, ctx, step0, st, sd0, what):
    """a twin walked straight to the step and rebuilt there: cost exactly 1.0, the tree hr_bvh_build_info_deformable predicts"""
    twin = hr.Scene(ctx, dc.with_verts(sd0, step0.verts), deformable=True)
    put(twin, st.verts)
    twin.rebuild()
    assert twin.refit_cost() == 1.0, (what, twin.refit_cost())
    info, host = twin.refresh_info(), hr.bvh_build_info(st.verts, deformable=True)
    assert (info.n_tris, info.n_nodes, info.max_depth, info.node_bytes, info.tri_bytes, info.box_pad) == (host.n_tris, host.n_nodes, host.max_depth, host.node_bytes, host.tri_bytes, host.box_pad), what
    assert list(info.bounds_lo) == list(host.bounds_lo) and list(info.bounds_hi) == list(host.bounds_hi), what
    twin.close()


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("name", list(dc.BASES))
def test_one_scene_through_a_hostile_stream(oracle, hr, ctx, name, family):
    sd0 = dc.BASES[name]()
    steps = dc.stream(name, family)
    g = hr.Scene(ctx, dc.with_verts(sd0, steps[0].verts), deformable=True)
    if family == "nonfinite":
        steps = dc.stream(name, family, leaf=a_leaf(g))     # (c) poisons a real leaf of this tree
    # what a scene that never saw the hostile steps holds after one refit over the base
    calm = hr.Scene(ctx, dc.with_verts(sd0, steps[0].verts), deformable=True)
    put(calm, sd0.verts)
    calm_nodes, calm_cost = calm.read_bvh()[0], calm.refit_cost()
    calm.close()
    uid = g.id
    for i, st in enumerate(steps):
        what = f"{name}/{family}/{i} {st.label}"
        put(g, st.verts)
        cost = g.refit_cost()
        assert cost == cost and cost >= 0.0, (what, cost)
        check_answers(hr, ctx, oracle, g, sd0, st, what, seed=i)
        check_boxes(g, dc.with_verts(sd0, st.verts), what)
        if len(dc.strip_nonfinite(st.verts)[0]):
            check_rebuild(hr, ctx, steps[0], st, sd0, what)
        if st.label == "back to the base":
            nodes = g.read_bvh()[0]
            diff = np.flatnonzero((nodes != calm_nodes).any(1))
            assert len(diff) == 0, f"{what}: {len(diff)} of {len(nodes)} nodes remember the hostile step, first {diff[:4]}"
            assert g.refit_cost() == calm_cost, what
    assert g.id == uid
    g.close()


@pytest.mark.parametrize("name", list(dc.BASES))
def test_a_poisoned_sub_range(oracle, hr, ctx, name):
    """nonfinite (a) through update_vertices(first_tri=...) over the poisoned triangle alone, restored through the same range: the answers of the
    full update, then the node bytes of before"""
    sd0 = dc.BASES[name]()
    steps = dc.stream(name, "nonfinite")
    g = hr.Scene(ctx, sd0, deformable=True)
    before, refs = g.read_bvh()
    t = dc.AIMED[name]
    for i, st in enumerate(steps[1:19], 1):     # the nine (a) steps, each followed by the base
        assert st.label.startswith("(a)") == bool(i & 1) and (st.label == "back to the base") == (not i & 1), st.label
        put(g, st.verts, first=t, count=1)
        what = f"{name}/sub-range/{i} {st.label}"
        check_answers(hr, ctx, oracle, g, sd0, st, what, seed=i)
        check_boxes(g, dc.with_verts(sd0, st.verts), what)
        if not i & 1:
            nodes, refs2 = g.read_bvh()
            assert np.array_equal(nodes, before) and np.array_equal(refs, refs2), f"{what}: the node bytes of before"
            assert g.refit_cost() == 1.0
    g.close()


# ---------------------------------------------------------------------------------------------------------------- shared instanced scenes
def mesh_entry(verts, bounds):
    e = dict(mesh_idx=0, positions=cuda(verts))
    if bounds == "exact":
        p = verts.reshape(-1, 3)
        e["bounds"] = (p.min(0), p.max(0))
    return e


def check_shared(hr, ctx, oracle, g, isd, st, what, seed):
    """the updated shared scene against hr_scene_create over flatten() of the step's data and against brute force; hit fractions as in
    tests/test_gpu_instances_shared_deform.py"""
    from hybrid_rendering_amd import api
    now = dc.shared_with(isd, st.verts)
    flat = now.flatten()
    sets = dc.shared_ray_sets(now, st, api.bvh_child_boxes(flat.verts), seed=seed)
    gf, osc = hr.Scene(ctx, flat), oracle.Scene(flat)
    hits = {}
    for name, rays in sets.items():
        rays = rays[dc.sound(osc, flat.verts, rays)]     # without the reference's hits by rounding alone
        a = answers(g, cuda(rays))
        assert_same(a, answers(gf, cuda(rays)), f"{what}/{name}: updated shared scene against the flattened scene")
        assert compare_with_brute_force(g, osc, rays, f"{what}/{name}") == 0
        hits[name] = (int(a[0].sum()), len(rays))
    gf.close()
    assert 0.10 <= hits["static"][0] / hits["static"][1] <= 0.90, (what, hits)
    if st.kind != "nothing":
        assert 0.10 <= sum(h for h, _ in hits.values()) / sum(n for _, n in hits.values()) <= 0.90, (what, hits)


@pytest.mark.parametrize("bounds", ["measured", "exact"])
@pytest.mark.parametrize("family", ["grow_point", "grow_seed", "shrink", "drift"])
def test_the_flagged_mesh_of_a_shared_scene_through_a_hostile_stream(oracle, hr, ctx, family, bounds):
    isd = dc.shared_scene()
    steps = dc.stream("heightfield16", family)
    g = hr.InstancedScene(ctx, dc.shared_with(isd, steps[0].verts), shared=True, deformable=dc.SHARED_FLAGS)
    for i, st in enumerate(steps):
        g.update_meshes([mesh_entry(st.verts, bounds)])
        cost = g.mesh_refit_cost(0)
        assert cost == cost, (st.label, cost)
        check_shared(hr, ctx, oracle, g, isd, st, f"shared/{family}/{bounds}/{i} {st.label}", seed=i)
    g.close()


def test_a_non_finite_mesh_is_reported_and_the_other_mesh_answers_as_before(oracle, hr, ctx):
    """nonfinite (a) and (e) on the flagged mesh with measured bounds: the documented error; rays too short to leave the static mesh's instance
    answer as before the call; a finite update afterwards brings the whole scene back to the flattened fresh scene"""
    isd = dc.shared_scene()
    steps = dc.stream("heightfield16", "nonfinite")
    g = hr.InstancedScene(ctx, isd, shared=True, deformable=dc.SHARED_FLAGS)
    flat = isd.flatten()
    first, _, _, count = isd.layout()
    box = flat.verts[first[2]:first[2] + count[2]].reshape(-1, 3).astype(np.float64)
    field = flat.verts[:first[2]].reshape(-1, 3).astype(np.float64)
    gap = np.maximum(np.maximum(field.min(0) - box.max(0), box.min(0) - field.max(0)), 0.0)
    reach = float(np.linalg.norm(gap))
    assert reach > 10.0, "the static mesh's instance stands clear of the field's"
    rng = np.random.RandomState(3)
    n = 4000
    o = rng.uniform(box.min(0), box.max(0), (n, 3))
    rays = rc.pack(o.astype(F32), rc.unit(rng.normal(size=(n, 3))), np.full(n, 0.9 * reach, F32), 0.0)
    before = answers(g, cuda(rays))
    assert 0.10 <= before[0].mean() <= 0.90
    assert compare_with_brute_force(g, oracle.Scene(flat), rays, "the static mesh's rays") == 0
    hostile = [s for s in steps if s.label.startswith("(a)") or s.label.startswith("(e)")]
    assert len(hostile) == 10
    for i, st in enumerate(hostile):
        with pytest.raises(hr.HRError, match=r"mesh 0 is not finite after the update"):
            g.update_meshes([mesh_entry(st.verts, "measured")])
        assert_same(answers(g, cuda(rays)), before, f"{st.label}: the static mesh's rays after the refused update")
        g.update_meshes([mesh_entry(steps[0].verts, "measured")])
        check_shared(hr, ctx, oracle, g, isd, steps[0], f"shared/after {st.label}", seed=i)
    g.close()


# ---------------------------------------------------------------------------------------------------------------- passes
def test_live_passes_over_bounds_that_no_longer_describe_the_scene(oracle, hr, ctx):
    """cornell32 created from the point placeholder; frame 0 the placeholder, 1 the real size, 2 drifted to 50000 on all axes (camera and light
    with it), 3 a -inf coordinate on the short box.  ONE live shadows pass (occluder cache) and ONE live AO pass (2 spp, entry-node table) trace
    every frame: masks and ray counts equal those of passes created for a scene created fresh for the frame, and (exact mode) the oracle's"""
    import torch
    W, H = 64, 48
    sd0 = synth.cornell32()
    base = sd0.verts
    off = np.asarray(dc.DRIFT_OFFSETS[1], F32)
    poisoned = base.copy()
    poisoned[dc.AIMED["cornell32"], 1, 0] = -np.inf
    frames = [(np.ascontiguousarray(np.broadcast_to(base[0, 0], base.shape)), 0), (base, 0), (base + off, 1), (poisoned, 0)]
    g = hr.Scene(ctx, dc.with_verts(sd0, frames[0][0]), deformable=True)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()

    def passes():
        ps = hr.RayTracedShadows(ctx, W, H), hr.RayTracedAO(ctx, W, H, 0)
        ps[1].params.spp = 2
        for p in ps:
            p.params.exact = 1
        return ps
    gs, ga = passes()
    os_, oa = oracle.ShadowsPass(W, H), oracle.AOPass(W, H, spp=2, zbp=synth.z_buffer_params())
    cam0, light0 = helpers.cameras("cornell", W / H, 1, 0.0)[0], helpers.light_for("cornell", "soft")
    mh = (H + 3) // 4
    prev = None
    n_rays = []
    for f, (verts, moved) in enumerate(frames):
        sd = dc.with_verts(sd0, verts)
        put(g, verts)
        shift = off.astype(np.float64) * moved
        cam = synth.Camera(tuple(np.asarray(cam0.eye) + shift), tuple(np.asarray(cam0.target) + shift), fov=cam0.fov, aspect=cam0.aspect)
        light = light0.copy()
        light[4:7] += (off * moved).astype(F32)
        ubo = synth.make_ubo(cam, None, light)
        osc, gf = oracle.Scene(sd), hr.Scene(ctx, sd)
        cur = osc.gbuffer(ubo, W, H)
        fi = hr.frame_inputs(helpers.to_cuda(cur), helpers.to_cuda(prev if prev is not None else cur), ubo, f, f & 1, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
        fs, fa = passes()
        gs.ray_trace(g, fi); ga.ray_trace(g, fi)
        fs.ray_trace(gf, fi); fa.ray_trace(gf, fi)
        os_.render(osc, ubo, cur, prev if prev is not None else cur, sob, sr, f)
        oa.render(osc, ubo, cur, prev if prev is not None else cur, sob, sr, f)
        torch.cuda.synchronize()
        ms, ma = gs.image(gs.IMG_MASK).cpu().numpy().view(np.uint32), ga.image(ga.IMG_MASK).cpu().numpy().view(np.uint32)
        assert np.array_equal(ms, fs.image(fs.IMG_MASK).cpu().numpy().view(np.uint32)), f"frame {f}: shadow mask, live pass on the live scene against a fresh pair"
        assert np.array_equal(ma, fa.image(fa.IMG_MASK).cpu().numpy().view(np.uint32)), f"frame {f}: AO masks, live pass on the live scene against a fresh pair"
        assert gs.ray_count() == fs.ray_count() and ga.ray_count() == fa.ray_count(), f"frame {f}: ray counts"
        assert np.array_equal(ms, os_.stages["mask"]), f"frame {f}: shadow mask against the oracle"
        assert np.array_equal(ma[:2 * mh].reshape(2, mh, -1), oa.stages["mask"]), f"frame {f}: AO masks against the oracle"
        n_rays.append((gs.ray_count(), ga.ray_count()))
        for p in (fs, fa, gf):
            p.close()
        prev = cur
    print("rays per frame (shadows, AO):", n_rays)
    assert n_rays[0] == (0, 0) and all(s > 0 and a > 0 for s, a in n_rays[1:]), n_rays
    for p in (gs, ga, g):
        p.close()
