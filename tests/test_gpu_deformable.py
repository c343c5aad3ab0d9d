"""Deformable scenes on the GPU (hr_scene_create_deformable / hr_scene_update_vertices / hr_scene_refit_cost / hr_scene_rebuild: csrc/deform.hip,
csrc/deform_refit.hip, csrc/refit.h).  The contract needs no tolerance: any-hit is a function of the triangle set, closest hit is the smallest t with ties to the smallest
triangle index, so a refitted tree answers bit for bit like hr_scene_create over the same vertices and like brute force; a refit with the creation
vertices reproduces the builder's node bytes, which pins the refit's encoding to bvh_build.cpp's."""
import numpy as np
import pytest

import helpers
import ray_cases as rc
from hybrid_rendering_amd import synth, synth_env
from test_gpu_instances import _rays
from test_gpu_instances_shared import answers, assert_same, compare_with_brute_force

pytestmark = pytest.mark.gpu

SCENES = {"cornell32": synth.cornell32, "heightfield64": lambda: synth.heightfield(64), "sponza_small": lambda: synth.sponza_like(detail=0.25)}
F32 = np.float32


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def update(g, sd, normals=True, first=0, count=None):
    count = sd.n_tris - first if count is None else count
    g.update_vertices(cuda(sd.verts[first:first + count]), cuda(sd.normals[first:first + count]) if normals else None, first_tri=first)


def scene_rays(verts, n, seed):
    """test_gpu_instances._rays (uniform origins, uniform directions, a quarter of them short) mapped from its unit cube into the scene's box grown
    by 5 %, lengths scaled with the diagonal"""
    lo, hi, diag = rc.scene_box(verts)
    r = _rays(n, seed, 0.0, 1.0)
    ext = np.maximum(hi - lo, 1e-3 * diag)
    r[:, :3] = ((lo - 0.05 * ext) + r[:, :3].astype(np.float64) * (1.1 * ext)).astype(F32)
    r[:, 3] = np.where(r[:, 3] >= 1e4, r[:, 3], r[:, 3] * F32(diag / 100.0)).astype(F32)
    r[:, 7] = F32(1e-4 * diag)
    return r


def own_boxes(g):
    """the child boxes of the scene's CURRENT node array, de-quantised as the traversal does (origin + q * 2^(e - 127), one rounding), as
    api.CHILD_BOX_DTYPE records — plus (leaf slots) tri_base + offset and count"""
    from hybrid_rendering_amd import api
    nodes, tris = g.read_bvh()
    n = len(nodes)
    o = nodes[:, 0:12].copy().view(F32).reshape(n, 3)
    e = nodes[:, 12:15].astype(np.uint32)
    counts = nodes[:, 15]
    child_base, tri_base = nodes[:, 16:20].copy().view(np.uint32)[:, 0], nodes[:, 20:24].copy().view(np.uint32)[:, 0]
    meta = nodes[:, 24:32]
    qlo, qhi = nodes[:, 32:56].reshape(n, 3, 8), nodes[:, 56:80].reshape(n, 3, 8)
    step = (e << 23).view(F32)
    depth = np.zeros(n, np.int32)
    out, leaf = [], []
    for j in range(n):
        ni, nc = int(counts[j]) & 15, int(counts[j]) >> 4
        depth[child_base[j]:child_base[j] + ni] = depth[j] + 1 if ni else 0
        for c in range(nc):
            lo = (qlo[j, :, c].astype(F32) * step[j] + o[j]).astype(F32)
            hi = (qhi[j, :, c].astype(F32) * step[j] + o[j]).astype(F32)
            out.append((lo, hi, step[j], j, c, depth[j], int(c >= ni)))
            leaf.append((int(tri_base[j]) + (int(meta[j, c]) & 31), int(meta[j, c]) >> 5) if c >= ni else (int(child_base[j]) + c, 0))
    return np.array(out, api.CHILD_BOX_DTYPE), np.array(leaf, np.int64).reshape(-1, 2), nodes, tris


def sample(boxes, k, seed):
    if len(boxes) <= k:
        return boxes
    return boxes[np.sort(np.random.RandomState(seed).permutation(len(boxes))[:k])]


def ray_sets(g, verts, seed, n_random=8000, n_boxes=100, n_tris=150):
    """the three families of the issue: uniform rays, grazers of the child boxes (a fresh tree's over the deformed vertices AND the refitted scene's own),
    rays through edges and vertices of the deformed triangles"""
    from hybrid_rendering_amd import api
    fresh = sample(api.bvh_child_boxes(verts), n_boxes, seed)
    own = sample(own_boxes(g)[0], n_boxes, seed + 1)
    return {"uniform": scene_rays(verts, n_random, seed),
            "box_grazers": rc.box_grazers(np.concatenate([fresh, own]), seed=seed + 2),
            "edge_and_vertex": rc.edge_and_vertex_rays(verts, seed=seed + 3, max_tris=n_tris)}


def check_queries(hr, ctx, oracle, g, sd, what, seed):
    """every ray set: the deformable scene against hr_scene_create over the same vertices and against brute force; hit fraction within [0.10, 0.90]"""
    osc, gf = oracle.Scene(sd), hr.Scene(ctx, sd)
    for name, rays in ray_sets(g, sd.verts, seed).items():
        assert_same(answers(g, cuda(rays)), answers(gf, cuda(rays)), f"{what}/{name}: refitted against a fresh scene")
        compare_with_brute_force(g, osc, rays, f"{what}/{name}")
        frac = float((osc.any_hit(rays, brute_force=True) != 0).mean())
        assert 0.10 <= frac <= 0.90, (what, name, frac)
    gf.close()


def check_boxes(g, sd, what):
    """The box invariants, on what hr_scene_read_bvh gives back.  A node stores its children's boxes QUANTISED on its own grid (origin = its exact
    lower corner, lo floored, hi ceiled), so a child's de-quantised child boxes may stand up to one of the CHILD's grid steps outside the parent's
    de-quantised slot — the builder's own trees do (131 of the 617 internal slots of the 64x64 heightfield as built, counted on the host through
    hr_bvh_child_boxes).  What the walk relies on, and what is asserted, exactly: with the TRUE box of a leaf = the fp32 bounds of its triangles
    -/+ the pad and the true box of a node = the union of its children's true boxes (recomputed here from the references read back),
      * every leaf slot's de-quantised box contains the leaf's true box (so every vertex, with the pad around it);
      * every internal slot's de-quantised box contains the child node's true box (so everything beneath it, at every level);
      * a child's de-quantised child boxes lie inside the parent's slot grown by ONE grid step of the child per axis on the upper side and not at
        all on the lower (the format's precision: floor / ceil on a grid whose origin is the child's exact lower corner);
      * hr_scene_get_info reports the numpy min / max of the vertices.
    Triangles with a NaN or infinite coordinate count for nothing, as in the builder: a leaf without a finite triangle and a node without a
    non-empty child are EMPTY — stored inverted (lo > hi on every axis) in their parent, outside every true box; a node that holds nothing has
    origin 0 — and the bounds reported are those of the finite triangles, 0 when there are none."""
    boxes, leaf, nodes, tris = own_boxes(g)
    info = g.refresh_info()
    pad = F32(info.box_pad)
    t = tris.reshape(-1, 48)
    prim = t[:, 12:16].copy().view(np.uint32)[:, 0]
    tv = np.stack([t[:, 0:12].copy().view(F32), t[:, 16:28].copy().view(F32), t[:, 32:44].copy().view(F32)], 1)   # [ref][3][3]
    assert np.array_equal(tv.view(np.uint32), sd.verts[prim].view(np.uint32)), f"{what}: the references hold the updated vertices"
    assert len(np.unique(prim)) == len(prim) == sd.n_tris, f"{what}: one reference per triangle"
    n = len(nodes)
    first_of_node, count_of_node = {}, {}
    for i, b in enumerate(boxes):
        first_of_node.setdefault(int(b["node"]), i)
        count_of_node[int(b["node"])] = count_of_node.get(int(b["node"]), 0) + 1
    true_lo, true_hi = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    slot_lo, slot_hi = np.zeros((len(boxes), 3), F32), np.zeros((len(boxes), 3), F32)   # true box of what every slot holds
    empty = np.zeros(len(boxes), bool)
    fin = np.isfinite(tv.reshape(len(tv), 9)).all(1)
    for j in sorted(first_of_node, reverse=True):   # children sit behind their parent
        k, c = first_of_node[j], count_of_node[j]
        for i in range(k, k + c):
            if boxes[i]["is_leaf"]:
                assert leaf[i, 1] > 0, f"{what}: an empty leaf (node {j})"
                v = tv[leaf[i, 0]:leaf[i, 0] + leaf[i, 1]][fin[leaf[i, 0]:leaf[i, 0] + leaf[i, 1]]].reshape(-1, 3)
                empty[i] = len(v) == 0
                if len(v):
                    slot_lo[i], slot_hi[i] = (v.min(0) - pad).astype(F32), (v.max(0) + pad).astype(F32)
            else:
                slot_lo[i], slot_hi[i] = true_lo[leaf[i, 0]], true_hi[leaf[i, 0]]
                empty[i] = not (true_lo[leaf[i, 0]] <= true_hi[leaf[i, 0]]).all()
        full = np.flatnonzero(~empty[k:k + c]) + k
        true_lo[j], true_hi[j] = (slot_lo[full].min(0), slot_hi[full].max(0)) if len(full) else (np.full(3, np.inf, F32), np.full(3, -np.inf, F32))
        assert np.array_equal(nodes[j, 0:12].copy().view(F32), true_lo[j] if len(full) else np.zeros(3, F32)), f"{what}: node {j}'s origin is not the lower corner of its true box"
    assert (boxes["lo"][empty] > boxes["hi"][empty]).all(), f"{what}: an empty slot is not stored inverted on every axis"
    holds = empty | ((boxes["lo"] <= slot_lo).all(1) & (boxes["hi"] >= slot_hi).all(1))
    assert holds.all(), f"{what}: {int((~holds).sum())} de-quantised slot boxes do not contain what they hold, first (node, slot) {boxes['node'][~holds][:4]}, {boxes['slot'][~holds][:4]}"
    for i, b in enumerate(boxes):
        if not b["is_leaf"] and not empty[i] and int(leaf[i, 0]) in first_of_node:
            k = first_of_node[int(leaf[i, 0])]
            kids = boxes[k:k + count_of_node[int(leaf[i, 0])]][~empty[k:k + count_of_node[int(leaf[i, 0])]]]
            assert (kids["lo"] >= b["lo"]).all() and (kids["hi"] <= (b["hi"] + kids["step"]).astype(F32)).all(), \
                f"{what}: a child box more than one grid step outside its parent's (node {b['node']} slot {b['slot']})"
    v = sd.verts[np.isfinite(sd.verts.reshape(sd.n_tris, 9)).all(1)].reshape(-1, 3)
    lo, hi = (v.min(0), v.max(0)) if len(v) else (np.zeros(3, F32), np.zeros(3, F32))
    assert list(info.bounds_lo) == list(lo) and list(info.bounds_hi) == list(hi), f"{what}: exact bounds after the update"


def test_refit_with_the_creation_vertices_reproduces_the_builders_nodes(hr, ctx):
    """the refit's encoding IS the builder's: same vertices in, the node array byte for byte as built, cost exactly 1.0"""
    for name, make in SCENES.items():
        sd = make()
        g = hr.Scene(ctx, sd, deformable=True)
        built, refs = g.read_bvh()
        assert g.refit_cost() == 1.0
        update(g, sd)
        nodes, refs2 = g.read_bvh()
        diff = np.flatnonzero((nodes != built).any(1))
        assert len(diff) == 0, f"{name}: {len(diff)} of {len(nodes)} nodes differ from the builder's after a refit over the same vertices, first {diff[:4]}"
        assert np.array_equal(refs, refs2)
        assert g.refit_cost() == 1.0, (name, g.refit_cost())
        info = g.refresh_info()
        host = hr.bvh_build_info(sd.verts, deformable=True)
        assert (info.n_nodes, info.max_depth, info.tri_bytes, list(info.bounds_lo), list(info.bounds_hi)) == (host.n_nodes, host.max_depth, host.tri_bytes, list(host.bounds_lo), list(host.bounds_hi))
        g.close()


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("kind", ["wave", "twist", "collapse"])
def test_queries_and_boxes_after_every_step(oracle, hr, ctx, name, kind):
    """5 steps of a deformation: after each, queries equal a fresh hr_scene_create over the deformed vertices and brute force on every ray set,
    and the refitted boxes hold their triangles and their children"""
    sd0 = SCENES[name]()
    g = hr.Scene(ctx, sd0, deformable=True)
    uid = g.id
    for step in range(1, 6):
        sd = synth.deform(sd0, step, kind)
        update(g, sd)
        check_queries(hr, ctx, oracle, g, sd, f"{name}/{kind}/{step}", seed=step)
        check_boxes(g, sd, f"{name}/{kind}/{step}")
    assert g.id == uid
    g.close()


def test_sub_range_updates(hr, ctx):
    """three disjoint ranges one after the other == one full update; a range updated and restored gives back the node bytes of before"""
    sd0 = synth.heightfield(64)
    sd = synth.deform(sd0, 3, "wave")
    n = sd.n_tris
    a, b = hr.Scene(ctx, sd0, deformable=True), hr.Scene(ctx, sd0, deformable=True)
    update(a, sd)
    cuts = [0, n // 5, n // 5 + 1, n]
    for i in (1, 2, 0):
        update(b, sd, first=cuts[i], count=cuts[i + 1] - cuts[i])
    (na, ta), (nb, tb) = a.read_bvh(), b.read_bvh()
    assert np.array_equal(na, nb) and np.array_equal(ta, tb)
    assert a.refit_cost() == b.refit_cost() and a.refit_cost() != 1.0
    sd2 = synth.deform(sd0, 4, "twist")
    update(b, sd2, first=1000, count=3000)
    assert not np.array_equal(b.read_bvh()[0], na)
    update(b, sd, first=1000, count=3000)
    (nb, tb) = b.read_bvh()
    assert np.array_equal(na, nb) and np.array_equal(ta, tb)
    assert list(a.refresh_info().bounds_lo) == list(b.refresh_info().bounds_lo)
    a.close(); b.close()


def level_widths(nodes):
    """nodes per depth of a tree read back by read_bvh(): children follow their parent in the builder's breadth-first order"""
    n_internal, child_base = nodes[:, 15] & 15, nodes[:, 16:20].copy().view(np.uint32)[:, 0]
    depth = np.zeros(len(nodes), np.int64)
    for j in range(len(nodes)):
        depth[int(child_base[j]):int(child_base[j]) + int(n_internal[j])] = depth[j] + 1
    return np.bincount(depth).tolist()


def test_a_flat_scene_and_a_one_mesh_shared_scene_refit_alike(hr, ctx):
    """One refit engine (csrc/deform_refit.hip) under two front ends: the same heightfield as a flat deformable scene (levels of up to 512 nodes in
    the one-workgroup launch) and as the only, flagged mesh of a shared instanced scene under one identity instance (up to 32).  heightfield(86) is
    the smallest whose split-free tree (levels of 1, 8, 64, 512, 515 and 2 nodes) has a level wider than 512 AND one of 33 to 512, so the per-level
    kernel and the one-workgroup kernel both run in both scenes and split the levels differently.  After every step the flat scene's nodes equal
    the mesh's subtree byte for byte (child_base of a node with internal children: less the subtree's root index), the references are equal, and
    the two cost ratios — double sums of the same half areas in different workgroup partitions, which agree to about n_nodes * 2^-53 relative,
    far below the 2^-24 of the rounding to float that follows the division — lie at most one float ulp apart; the creation vertices give exactly 1.0."""
    sd0 = synth.heightfield(86)
    isd = synth.InstancedSceneData(meshes=[sd0], instances=[(np.eye(4, dtype=F32).reshape(16), 0, 1)], materials=sd0.materials)
    a, b = hr.Scene(ctx, sd0, deformable=True), hr.InstancedScene(ctx, isd, shared=True, deformable=[1])
    widths = level_widths(a.read_bvh()[0])
    print(f"{sd0.n_tris} triangles, nodes per level {widths}")
    assert max(widths) > 512 and any(33 <= w <= 512 for w in widths), widths
    root = len(b.read_bvh()[0]) - len(a.read_bvh()[0])
    assert root >= 1

    def both(sd, first=0, count=None):
        count = sd.n_tris - first if count is None else count
        update(a, sd, first=first, count=count)
        b.update_meshes([dict(mesh_idx=0, positions=cuda(sd.verts[first:first + count]), normals=cuda(sd.normals[first:first + count]), first_tri=first)])

    def compare(what):
        (na, ta), (nb, tb) = a.read_bvh(), b.read_bvh()
        nb = nb[root:].copy()
        shifted = nb[:, 16:20].copy().view(np.uint32) - np.where(nb[:, 15:16] & 15, np.uint32(root), np.uint32(0)).astype(np.uint32)
        nb[:, 16:20] = shifted.view(np.uint8)
        diff = np.flatnonzero((na != nb).any(1))
        assert len(diff) == 0, f"{what}: {len(diff)} of {len(na)} nodes differ between the two scenes, first {diff[:4]}"
        assert np.array_equal(ta, tb), f"{what}: the references differ"
        ca, cb = np.float32(a.refit_cost()), np.float32(b.mesh_refit_cost(0))
        print(f"{what}: cost ratio flat {ca!r}, shared {cb!r}")
        assert abs(int(ca.view(np.int32)) - int(cb.view(np.int32))) <= 1, (what, ca, cb)
        return na, ca, cb

    built, ca, cb = compare("as built")
    assert ca == 1.0 and cb == 1.0
    both(sd0)
    nodes, ca, cb = compare("the creation vertices")
    assert np.array_equal(nodes, built) and ca == 1.0 and cb == 1.0
    for step, kind in ((1, "wave"), (2, "twist"), (3, "collapse")):
        both(synth.deform(sd0, step, kind))
        nodes, ca, cb = compare(f"{kind} {step}")
        assert ca != 1.0 and not np.array_equal(nodes, built)
    both(synth.deform(sd0, 2, "wave"), first=1000, count=3001)   # a sub-range that is no multiple of the scatter's 256 triangles per workgroup
    compare("a sub-range of wave 2 over collapse 3")
    both(sd0)
    nodes, ca, cb = compare("the creation vertices again")
    assert np.array_equal(nodes, built) and ca == 1.0 and cb == 1.0
    a.close(); b.close()


def _pass_images(gs, ga, gd, gr, gt, hr):
    import torch
    irr, dep = gd.current_read()
    return {"shadow mask": gs.image(gs.IMG_MASK), "shadows temporal": gs.output(hr.OUTPUT_TEMPORAL_ACCUMULATION), "shadows denoised": gs.output(hr.OUTPUT_ATROUS),
            "AO masks": ga.image(ga.IMG_MASK), "AO denoised": ga.output(),
            "DDGI radiance": gd.image(gd.IMG_RADIANCE), "DDGI direction / distance": gd.image(gd.IMG_DIRDIST), "DDGI irradiance": irr, "DDGI depth": dep,
            "reflections trace": gr.image(gr.IMG_TRACE), "reflections denoised": gr.output(hr.OUTPUT_ATROUS), "ground truth": gt.output()}


@pytest.mark.parametrize("exact", [1, 0])
def test_passes_on_a_deforming_scene(oracle, hr, ctx, exact):
    """4 frames of "wave" on cornell32 at 160x120 and a fifth in which ONLY the normals change: every stage image of shadows, AO (2 spp), DDGI
    (3x3x3 probes, 32 rays), reflections (mirrors everywhere) and the ground truth on the deformable scene equals the one on a scene created fresh
    for the frame; in exact mode the masks, the DDGI radiance, the reflections trace image and the denoised outputs equal the oracle's too"""
    import dataclasses
    import torch
    from hybrid_rendering_amd import api_gi, api_reflections, api_post
    from oracle import pyoracle_ddgi as od, pyoracle_reflections as orf
    W, H = 160, 120
    sd0 = synth.cornell32()
    g = hr.Scene(ctx, sd0, deformable=True)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    lo, hi = sd0.bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 3, 3), rays_per_probe=32, normal_bias=1.0)
    sky = synth_env.sky_cubemap(16)
    pre, lut = synth_env.prefiltered_chain(sky, 5), synth_env.brdf_lut(16)
    env_np = dict(sky=sky, prefiltered=pre, pre_size=16, pre_levels=5, lut=lut)
    f16 = lambda a: torch.from_numpy(a).cuda().view(torch.float16)
    env = api_gi.environment(f16(sky), f16(pre), 16, 5, f16(lut))

    def make():
        ps = [hr.RayTracedShadows(ctx, W, H), hr.RayTracedAO(ctx, W, H, 0), api_gi.DDGI(ctx, W, H, ddgi), api_reflections.RayTracedReflections(ctx, W, H, 0),
              api_post.GroundTruthPathTracer(ctx, W, H)]
        ps[1].params.spp = 2
        for p in ps[:4]:
            p.params.exact = exact
        return ps
    A, B = make(), make()
    os_, oa = oracle.ShadowsPass(W, H), oracle.AOPass(W, H, spp=2, zbp=synth.z_buffer_params())
    odd, orr = od.DDGIPass(ddgi), orf.ReflectionsPass(W, H)
    cams = helpers.cameras("cornell", W / H, 6, 1.0)
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(2)
    prev_np, last_trace = None, None
    for f in range(5):
        sd = synth.deform(sd0, min(f + 1, 4), "wave")
        if f == 4:   # the vertices of frame 3, every normal tilted: only shading may change
            tilt = sd.normals + np.float32(0.6) * np.roll(sd.normals, 1, axis=2)
            sd = dataclasses.replace(sd, normals=(tilt / np.linalg.norm(tilt, axis=2, keepdims=True)).astype(np.float32))
            nodes_before = g.read_bvh()[0]
        update(g, sd)
        if f == 4:
            assert np.array_equal(g.read_bvh()[0], nodes_before)
        gf, osc = hr.Scene(ctx, sd), oracle.Scene(sd)
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur_a, cur_b, cur = g.gbuffer(ubo, W, H), gf.gbuffer(ubo, W, H), osc.gbuffer(ubo, W, H)
        for k in cur:
            got = cur_a[k].cpu().numpy()
            assert torch.equal(cur_a[k], cur_b[k]), f"frame {f}: G-buffer {k}, deformable against fresh"
            assert np.array_equal(got.view(np.uint16) if got.dtype == np.float16 else got, cur[k]), f"frame {f}: G-buffer {k} against the oracle"
        ch = cur["gb3"][..., 0]
        ch[ch == np.float16(0.8).view(np.uint16)] = np.float16(0.03).view(np.uint16)   # mirrors everywhere
        cur_d = helpers.to_cuda(cur)
        prev = prev_np if prev_np is not None else cur
        fi = hr.frame_inputs(cur_d, helpers.to_cuda(prev), ubo, f, f & 1, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
        orient = synth_env.random_orientation(rng)
        for (gs, ga, gd, gr, gt), scene in ((A, g), (B, gf)):
            gs.render(scene, fi); ga.render(scene, fi); gd.render(scene, fi, env, orient); gr.render(scene, fi, env, gd); gt.render(scene, ubo, env)
        torch.cuda.synchronize()
        ia, ib = _pass_images(*A, hr), _pass_images(*B, hr)
        for k in ia:
            assert torch.equal(ia[k], ib[k]), f"frame {f} (exact {exact}): {k} on the deformable scene differs from the fresh scene's"
        if f == 4:
            assert not torch.equal(ia["reflections trace"], last_trace), "the updated normals did not reach the hit shading"
        last_trace = ia["reflections trace"].clone()
        if exact:
            os_.render(osc, ubo, cur, prev, sob, sr, f)
            oa.render(osc, ubo, cur, prev, sob, sr, f)
            odd.render(osc, ubo, cur, sky, orient, f)
            irr, dep = odd.current_read()
            orr.render(osc, ubo, ddgi, cur, prev, sob, sr, f, env_np, irr, dep, ping_pong=bool(f & 1))
            mh = (H + 3) // 4
            assert np.array_equal(ia["shadow mask"].cpu().numpy().view(np.uint32), os_.stages["mask"]), f"frame {f}: shadow mask against the oracle"
            assert np.array_equal(helpers.bits16(ia["shadows denoised"]), os_.stages["output"]), f"frame {f}: denoised shadows"
            assert np.array_equal(ia["AO masks"].cpu().numpy().view(np.uint32)[:2 * mh].reshape(2, mh, -1), oa.stages["mask"]), f"frame {f}: AO masks"
            assert np.array_equal(helpers.bits16(ia["DDGI radiance"]), odd.stages["radiance"]), f"frame {f}: DDGI radiance"
            assert np.array_equal(helpers.bits16(ia["reflections trace"]), orr.stages["trace"]), f"frame {f}: reflections trace image"
            assert np.array_equal(helpers.bits16(ia["reflections denoised"]), orr.stages["atrous"][-1]), f"frame {f}: denoised reflections"
        gf.close()
        prev_np = cur
    for p in A + B + [g]:
        p.close()


def test_pass_caches_notice_an_update(oracle, hr, ctx):
    """the AO pass object (entry-node table keyed on the scene and its geometry epoch) and the shadows pass (occluder cache: an index into the
    references, tested against the CURRENT vertices) live across an update that moves the short box across the room: masks equal the oracle's"""
    import torch
    W, H = 160, 120
    sd0 = synth.cornell32()
    g = hr.Scene(ctx, sd0, deformable=True)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    gs, ga = hr.RayTracedShadows(ctx, W, H), hr.RayTracedAO(ctx, W, H, 0)
    ga.params.spp = 2
    os_, oa = oracle.ShadowsPass(W, H), oracle.AOPass(W, H, spp=2, zbp=synth.z_buffer_params())
    cam, light = helpers.cameras("cornell", W / H, 1, 0.0)[0], helpers.light_for("cornell", "soft")
    ubo = synth.make_ubo(cam, None, light)
    prev = None
    for f, shift in enumerate(((0, 0, 0), (-38, 0, -30), (-38, 25, -30), (0, 0, 0))):
        v = sd0.verts.copy()
        v[20:30] += np.asarray(shift, np.float32)   # the short box: many AO grid cells away from where the table was built
        sd = synth.SceneData(v, sd0.normals, sd0.tri_material, sd0.tri_mesh_id, sd0.materials)
        update(g, sd, normals=False)
        osc = oracle.Scene(sd)
        cur = osc.gbuffer(ubo, W, H)
        fi = hr.frame_inputs(helpers.to_cuda(cur), helpers.to_cuda(prev if prev is not None else cur), ubo, f, f & 1, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
        gs.render(g, fi); ga.render(g, fi)
        os_.render(osc, ubo, cur, prev if prev is not None else cur, sob, sr, f)
        oa.render(osc, ubo, cur, prev if prev is not None else cur, sob, sr, f)
        torch.cuda.synchronize()
        mh = (H + 3) // 4
        assert np.array_equal(gs.image(gs.IMG_MASK).cpu().numpy().view(np.uint32), os_.stages["mask"]), f"frame {f}: shadow mask (occluder cache across an update)"
        assert np.array_equal(ga.image(ga.IMG_MASK).cpu().numpy().view(np.uint32)[:2 * mh].reshape(2, mh, -1), oa.stages["mask"]), f"frame {f}: AO masks (entry table across an update)"
        prev = cur
    for p in (gs, ga, g):
        p.close()


def test_cost_and_rebuild(oracle, hr, ctx):
    """a twist costs box area; hr_scene_rebuild brings the cost back to 1.0, keeps the scene id and the answers, and builds the tree
    hr_bvh_build_info_deformable predicts for the current vertices"""
    sd0 = synth.sponza_like(detail=0.25)
    g = hr.Scene(ctx, sd0, deformable=True)
    uid = g.id
    sd = synth.deform(sd0, 5, "twist")
    update(g, sd)
    cost = g.refit_cost()
    print(f"refit cost after 5 steps of twist: {cost:.4f}")
    assert cost > 1.0
    check_queries(hr, ctx, oracle, g, sd, "twisted, refitted", seed=11)
    g.rebuild()
    assert g.refit_cost() == 1.0 and g.id == uid
    info, host = g.refresh_info(), hr.bvh_build_info(sd.verts, deformable=True)
    assert (info.n_tris, info.n_nodes, info.max_depth, info.node_bytes, info.tri_bytes, info.box_pad) == (host.n_tris, host.n_nodes, host.max_depth, host.node_bytes, host.tri_bytes, host.box_pad)
    assert list(info.bounds_lo) == list(host.bounds_lo) and list(info.bounds_hi) == list(host.bounds_hi)
    check_queries(hr, ctx, oracle, g, sd, "twisted, rebuilt", seed=11)
    check_boxes(g, sd, "rebuilt")
    built = g.read_bvh()[0]
    update(g, sd)   # and the rebuilt scene refits like a created one
    assert np.array_equal(g.read_bvh()[0], built) and g.refit_cost() == 1.0
    sd2 = synth.deform(sd0, 2, "wave")
    update(g, sd2)
    check_queries(hr, ctx, oracle, g, sd2, "rebuilt, then waved", seed=12)
    g.close()


def test_errors_enqueue_nothing(hr, ctx):
    """a plain scene, an instanced scene, a range past the end, a null positions: HR_ERR_INVALID_ARG with a message naming the call, node bytes as before"""
    import ctypes as C
    import torch
    L = hr.lib()
    L.hr_scene_update_vertices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    sd = synth.cornell32()
    plain, inst, g = hr.Scene(ctx, sd), hr.InstancedScene(ctx, synth.instanced_cornell(3, seed=1)), hr.Scene(ctx, sd, deformable=True)
    pos = cuda(synth.deform(sd, 2, "wave").verts)
    p, n = C.c_void_p(pos.data_ptr()), sd.n_tris
    cases = [("a plain scene", plain, p, 0, n), ("an instanced scene", inst, p, 0, n), ("a range past the end", g, p, 1, n), ("a negative start", g, p, -1, 4),
             ("null positions", g, None, 0, n)]
    for what, scene, ptr, first, count in cases:
        before = scene.read_bvh()[0]
        st = L.hr_scene_update_vertices(scene.h, ptr, None, first, count, None)
        msg = L.hr_last_error().decode()
        assert st == 1 and "hr_scene_update_vertices" in msg, (what, st, msg)
        torch.cuda.synchronize()
        assert np.array_equal(scene.read_bvh()[0], before), f"{what}: the node array changed"
    r = C.c_float(0)
    assert L.hr_scene_refit_cost(plain.h, C.byref(r)) == 1 and "hr_scene_refit_cost" in L.hr_last_error().decode()
    assert L.hr_scene_rebuild(inst.h, None) == 1 and "hr_scene_rebuild" in L.hr_last_error().decode()
    with pytest.raises(hr.HRError):
        plain.update_vertices(pos)
    for s in (plain, inst, g):
        s.close()


def test_hybrid_frame_over_a_scene_updated_between_frames(hr, ctx):
    """hr_hybrid_frame in streams and in graph mode over a deformable scene whose vertices change between frames: every pass output of every
    frame equals the plain serial render() calls of a twin set of passes (the comparison of tests/test_gpu_edge.py, with a moving BVH under it)"""
    import torch
    from hybrid_rendering_amd.frame import HybridFrame
    sd0 = synth.sponza_like(0.25)
    scene = hr.Scene(ctx, sd0, deformable=True)
    ref = HybridFrame(ctx, scene, sd0, 328, 184, probes=(5, 3, 4), rays_per_probe=64)
    twin = HybridFrame(ctx, scene, sd0, 328, 184, probes=(5, 3, 4), rays_per_probe=64)
    modes = ["graph", "graph", "streams", "graph", "serial", "graph", "streams", "graph"]
    for k, mode in enumerate(modes):
        update(scene, synth.deform(sd0, k, ("wave", "twist")[k & 1]))
        ref.render(k)
        twin.concurrent_streams(True, mode)
        twin.render(k)
        torch.cuda.synchronize()
        for n, p in ref.passes().items():
            assert torch.equal(p.output(), twin.passes()[n].output()), f"frame {k} ({mode}): {n} output differs from the serial render() calls"
    ref.close(); twin.close(); scene.close()
