"""The device re-deal of a deformable mesh's triangles (hr_scene_rebuild_device / hr_scene_rebuild_meshes_device: csrc/deform_redeal.hip,
csrc/device_sort.h).  The node topology stands as the host built it; the triangles are sorted by the Morton code of their box and dealt in that
order to the tree's reference slots in depth-first order, then the standing refit runs.  No tolerance anywhere: the ORDER is the argsort of keys a
host function gives (hr_shared_top_sort_keys over the triangle boxes inside the exact bounds of the mesh's finite references), the TREE is what the
standing refit makes of the permuted references, and the ANSWERS are those of a fresh hr_scene_create over the same vertices and of brute force.

Sizes: 1 and 9 triangles (one node, two levels), 4096 and 4097 (the last size of the one-workgroup LDS sort, the first of the radix sort), 21218
(the radix sort over 83 tiles, and a bottom level wider than the 512 nodes of the one-workgroup refit): slices of one heightfield, whose first
half are the lower-left triangles of its cells in row-major order — neither Morton nor depth-first order.  The brute-force rounds run on the whole
64 x 64 field (8192 triangles, the radix path; the neighbouring tests' hit fractions hold for it) and at the hostile streams' 512; at 21218 one
round (8000 x 21218 triangle tests per ray set on the CPU is the cost that matters)."""
import ctypes as C

import numpy as np
import pytest

import deform_cases as dc
import helpers
import ray_cases as rc
import shared_deform_cases as sc
from hybrid_rendering_amd import synth
from test_gpu_deform_edges import check_answers, put
from test_gpu_deformable import check_queries, cuda, update
from test_gpu_deformable import scene_rays
from test_gpu_instances_shared import answers, assert_same, compare_with_brute_force
from test_gpu_instances_shared_deform import entry
from test_gpu_motion_vectors import assert_images_equal, images, ubo_for

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (1, 9, 4096, 4097, 21218)
FIELD, BOX = sc.FIELD, sc.BOX


def first_tris(sd, n):
    assert sd.n_tris >= n
    return synth.SceneData(np.ascontiguousarray(sd.verts[:n]), np.ascontiguousarray(sd.normals[:n]), sd.tri_material[:n], sd.tri_mesh_id[:n], sd.materials, f"{sd.name}[:{n}]")


_FIELDS = {}


def field(n):
    """the first n triangles of a heightfield: 64 x 64 cells up to 8192 triangles, 103 x 103 (21218 triangles) beyond"""
    if n not in _FIELDS:
        _FIELDS[n] = first_tris(synth.heightfield(64 if n <= 8192 else 103), n)
    return _FIELDS[n]


def walk(nodes, root=0):
    """the tree's reference slots depth-first, in numpy over csrc/bvh.h's layout: a node's internal slots (0 .. n_internal - 1: node child_base +
    slot) first, then its leaf slots in slot order, a leaf's triangles tri_base + offset .. + count - 1 in that order"""
    counts = nodes[:, 15]
    child_base, tri_base = nodes[:, 16:20].copy().view(np.uint32)[:, 0], nodes[:, 20:24].copy().view(np.uint32)[:, 0]
    meta = nodes[:, 24:32]
    out, stack = [], [(root, 0)]
    while stack:
        j, c = stack.pop()
        ni, nc = int(counts[j]) & 15, int(counts[j]) >> 4
        if c >= nc:
            continue
        stack.append((j, c + 1))
        if c < ni:
            stack.append((int(child_base[j]) + c, 0))
        else:
            m = int(meta[j, c])
            out.extend(range(int(tri_base[j]) + (m & 31), int(tri_base[j]) + (m & 31) + (m >> 5)))
    return np.asarray(out, np.int64)


def refs_of(tris):
    """(prim [m], vertices [m][3][3]) of triangle references read back"""
    t = tris.reshape(-1, 48)
    return t[:, 12:16].copy().view(np.uint32)[:, 0].astype(np.int64), np.stack([t[:, 0:12].copy().view(F32), t[:, 16:28].copy().view(F32), t[:, 32:44].copy().view(F32)], 1)


def expected_order(hr, verts, ref_verts):
    """argsort of the keys the re-deal sorts by: hr_shared_top_sort_keys of the triangles' boxes inside the exact bounds of the FINITE references
    the mesh holds when the call is made (`ref_verts`; none: the zero box), (1 << 62) | triangle for a triangle with a non-finite coordinate"""
    verts = np.asarray(verts, F32)
    n = len(verts)
    fin = dc.finite_mask(verts) if n else np.zeros(0, bool)
    rf = ref_verts[dc.finite_mask(ref_verts)].reshape(-1, 3) if len(ref_verts) else np.zeros((0, 3), F32)
    bounds = np.concatenate([rf.min(0), rf.max(0)]) if len(rf) else np.zeros(6, F32)
    boxes = np.zeros((n, 6), F32)
    boxes[fin, :3], boxes[fin, 3:] = verts[fin].min(1), verts[fin].max(1)
    keys = hr.shared_top_sort_keys(boxes, bounds)
    keys[~fin] = (np.uint64(1) << np.uint64(62)) | np.flatnonzero(~fin).astype(np.uint64)
    assert len(np.unique(keys)) == n
    return np.argsort(keys, kind="stable")


def check_order(hr, g, verts, ref_verts, what, root=0, ref_base=0):
    """the prim of the r-th reference of the tree read back, depth-first, is the r-th triangle of the expected order; returns (nodes, references)"""
    nodes, tris = g.read_bvh()
    prim, tv = refs_of(tris)
    slots = walk(nodes, root)
    order = expected_order(hr, verts, ref_verts)
    assert len(slots) <= len(order), what
    got = prim[slots]
    bad = np.flatnonzero(got != order[:len(slots)])
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(slots)} references out of Morton order, first ranks {bad[:4]}: triangles {got[bad[:4]]} for {order[bad[:4]]}"
    assert np.array_equal(tv[slots].view(np.uint32), np.asarray(verts, F32)[got].view(np.uint32)), f"{what}: a reference does not hold its triangle's vertices"
    return nodes, tris


def current_refs(g, first=0, count=None):
    _, tv = refs_of(g.read_bvh()[1])
    return tv[first:] if count is None else tv[first:first + count]


@pytest.mark.parametrize("n", SIZES)
def test_order_permutation_and_idempotence(hr, ctx, n):
    """(1) the order, (2) re-deal == permutation + the standing refit, on a twin, (3) a second re-deal changes nothing — at every size"""
    sd0 = field(n)
    sd = synth.deform(sd0, 2, "twist")
    g, twin = hr.Scene(ctx, sd0, deformable=True), hr.Scene(ctx, sd0, deformable=True)
    created_nodes, created_tris = g.read_bvh()
    update(g, sd)
    before = g.device_rebuild_counts()
    g.rebuild_device()
    nodes, tris = check_order(hr, g, sd.verts, sd.verts, f"{n} triangles")
    topo = slice(15, 32)                         # counts, child_base, tri_base, meta
    assert np.array_equal(nodes[:, topo], created_nodes[:, topo]), "the topology stands as the host built it"
    prim, tv = refs_of(tris)
    assert len(prim) == n and len(np.unique(prim)) == n
    # (2) the twin keeps the creation assignment: its slot s holds triangle q_s; hand q_s the vertices standing in slot s of the re-dealt scene
    q, _ = refs_of(created_tris)
    w = np.zeros_like(sd.verts)
    w[q] = tv
    twin.update_vertices(cuda(w))
    tn, tt = twin.read_bvh()
    assert np.array_equal(tn, nodes), f"{int((tn != nodes).any(1).sum())} of {len(nodes)} nodes differ from permutation + refit"
    same = np.ones(48, bool)
    same[12:16] = False
    assert np.array_equal(tt[:, same], tris[:, same]) and (n < 2 or not np.array_equal(tt, tris))
    assert twin.refit_cost() == g.refit_cost()
    # (3)
    cost = g.refit_cost()
    g.rebuild_device()
    nodes2, tris2 = g.read_bvh()
    assert np.array_equal(nodes2, nodes) and np.array_equal(tris2, tris) and g.refit_cost() == cost
    after = g.device_rebuild_counts()
    assert after["rebuilds_enqueued"] == before["rebuilds_enqueued"] + 2
    g.close(); twin.close()


def test_answers_through_updates_and_a_host_rebuild(oracle, hr, ctx):
    """(4) at 8192 triangles (the whole 64 x 64 field, on the radix path): after the re-deal, after a further full update, after a further sub-range update (a stale triangle -> reference map
    would scatter it into another triangle's slot), after a host rebuild followed by another re-deal"""
    sd0 = field(8192)
    n = sd0.n_tris
    g = hr.Scene(ctx, sd0, deformable=True)
    s1, s2, s3 = synth.deform(sd0, 3, "twist"), synth.deform(sd0, 2, "wave"), synth.deform(sd0, 4, "wave")
    update(g, s1)
    g.rebuild_device()
    check_queries(hr, ctx, oracle, g, s1, "re-dealt", seed=1)
    update(g, s2)
    check_queries(hr, ctx, oracle, g, s2, "re-dealt, then a full update", seed=2)
    first, count = n // 5, n // 3
    mixed = dc.with_verts(s2, s2.verts.copy())
    mixed.verts[first:first + count] = s3.verts[first:first + count]
    update(g, mixed, normals=False, first=first, count=count)
    nodes, tris = g.read_bvh()
    prim, tv = refs_of(tris)
    assert np.array_equal(tv.view(np.uint32), mixed.verts[prim].view(np.uint32)), "a sub-range update after a re-deal reaches the triangles' own references"
    check_queries(hr, ctx, oracle, g, mixed, "re-dealt, then a sub-range update", seed=3)
    g.rebuild()
    assert g.refit_cost() == 1.0
    update(g, s1)
    g.rebuild_device()
    check_order(hr, g, s1.verts, s1.verts, "host rebuild, then a re-deal")
    check_queries(hr, ctx, oracle, g, s1, "host rebuild, then a re-deal", seed=4)
    g.rebuild()
    assert g.refit_cost() == 1.0, "a host rebuild after a device re-deal"
    g.close()


def test_answers_at_the_radix_size(oracle, hr, ctx):
    """(4) once at 21218 triangles: the radix sort's order feeds a tree whose bottom level takes the per-level refit launches"""
    sd0 = field(21218)
    sd = synth.deform(sd0, 2, "wave")
    g = hr.Scene(ctx, sd0, deformable=True)
    update(g, sd)
    g.rebuild_device()
    check_queries(hr, ctx, oracle, g, sd, "21218 triangles re-dealt", seed=5)
    g.close()


def test_passes_do_not_notice(hr, ctx):
    """(5) shadows mask, AO masks and the motion G-buffer, 64 x 48, two frames on two scenes of which one is re-dealt between the frames: every image
    equal, so neither the shadow pass's state, nor the AO entry table keyed on the geometry epoch, nor the motion path holds a stale reference"""
    import torch
    w, h = 64, 48
    rest = synth.instanced_cornell(9, seed=5).flatten()
    moved = synth.deform(rest, 1, "wave")
    a, b = hr.Scene(ctx, rest, deformable=True), hr.Scene(ctx, rest, deformable=True)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    zbp = synth.z_buffer_params()
    passes = [(hr.RayTracedShadows(ctx, w, h), hr.RayTracedAO(ctx, w, h, 0)) for _ in (a, b)]
    for gs, ga in passes:
        gs.params.exact = ga.params.exact = 1
        ga.params.spp = 2
    prev = [None, None]
    for f in range(2):
        ubo = ubo_for(f, True, w, h)
        out = []
        for k, (g, (gs, ga)) in enumerate(zip((a, b), passes)):
            g.motion_begin_frame()
            if f == 0:
                g.update_vertices(cuda(moved.verts), cuda(moved.normals))
            elif k == 1:
                g.rebuild_device()
            cur = images(g.gbuffer(ubo, w, h, motion=True))
            prv = prev[k] if prev[k] is not None else cur
            fi = hr.frame_inputs(helpers.to_cuda(cur), helpers.to_cuda(prv), ubo, f, f & 1, sob_d, sr_d, z_buffer_params=zbp)
            gs.render(g, fi)
            ga.render(g, fi)
            torch.cuda.synchronize()
            out.append((cur, gs.image(gs.IMG_MASK).cpu().numpy().copy(), ga.image(ga.IMG_MASK).cpu().numpy().copy(), helpers.bits16(ga.image(ga.IMG_AO1 if f & 1 else ga.IMG_AO0)).copy(),
                        helpers.bits16(gs.output(hr.OUTPUT_ATROUS)).copy()))
            prev[k] = cur
        assert_images_equal(out[1][0], out[0][0], f"frame {f}: motion G-buffer")
        for x, y, name in zip(out[0][1:], out[1][1:], ("shadow mask", "AO masks", "temporal AO", "denoised shadows")):
            assert np.array_equal(x, y), f"frame {f}: {name} differs after a re-deal"
        if f == 0:
            lit = float(np.unpackbits(out[0][1].view(np.uint8)).mean())
            assert 0.02 < lit < 0.98, lit
    assert b.device_rebuild_counts()["rebuilds_enqueued"] == 1 and a.device_rebuild_counts()["rebuilds_enqueued"] == 0
    for gs, ga in passes:
        gs.close(); ga.close()
    a.close(); b.close()


def _hostile_cases():
    """(label, creation vertices, current vertices, poisoned now) over heightfield16's 512 triangles, from the generators of deform_cases.py"""
    base = np.ascontiguousarray(dc.BASES["heightfield16"]().verts, F32)
    aimed = dc.AIMED["heightfield16"]
    d5 = next(s for s in dc.nonfinite(base, aimed, seed=5) if s.label.startswith("(d)"))
    d6 = next(s for s in dc.nonfinite(base, aimed, seed=6) if s.label.startswith("(d)"))
    e5 = next(s for s in dc.nonfinite(base, aimed, seed=5) if s.label.startswith("(e)"))
    shrink = {s.label: s for s in dc.shrink(base)}
    return [("non-finite at creation, others now", d5.verts, d6.verts, d6.poisoned),
            ("non-finite at creation, all finite now", d5.verts, base, ()),
            ("30 % non-finite now", base, d5.verts, d5.poisoned),
            ("every triangle non-finite now", base, e5.verts, e5.poisoned),
            ("all triangles identical", base, np.ascontiguousarray(np.broadcast_to(base[aimed], base.shape)), ()),
            ("flat in one axis", base, shrink["plane"].verts, ()),
            ("collapsed to a point", base, shrink["point"].verts, ())]


def _held_step(label, verts, prim):
    """what the scene can answer for: the triangles that hold a reference — one that holds none (more finite triangles than the tree has slots:
    some were not finite when it was built) is out until the next re-deal or host build, as if it were not finite"""
    held = np.zeros(len(verts), bool)
    held[prim] = True
    visible = np.ascontiguousarray(np.where(held[:, None, None], np.asarray(verts, F32), F32(np.nan)))
    return dc.step_of(label, visible, np.flatnonzero(~dc.finite_mask(visible)))


@pytest.mark.parametrize("case", range(7))
def test_hostile_streams(oracle, hr, ctx, case):
    """(6) the order and the answers; every slot stays occupied: the finite triangles first, as many as there are slots, then non-finite ones"""
    label, created, now, poisoned = _hostile_cases()[case]
    sd0 = dc.BASES["heightfield16"]()
    n = len(now)
    g = hr.Scene(ctx, dc.with_verts(sd0, created), deformable=True)
    n_refs = int(dc.finite_mask(created).sum())
    put(g, now)
    ref_verts = current_refs(g)
    assert len(ref_verts) == n_refs
    g.rebuild_device()
    nodes, tris = check_order(hr, g, now, ref_verts, label)
    prim, tv = refs_of(tris)
    n_finite = int(dc.finite_mask(now).sum())
    assert len(prim) == n_refs and len(np.unique(prim)) == n_refs, f"{label}: every slot holds a triangle of its own"
    held_finite = int(dc.finite_mask(now)[prim].sum())
    assert held_finite == min(n_refs, n_finite) and n_refs - held_finite == max(0, n_refs - n_finite), label
    check_answers(hr, ctx, oracle, g, sd0, _held_step(label, now, prim), label, seed=case)
    # a sub-range update over the re-dealt map, back to the base: it must reach the slots the triangles hold NOW
    base = np.ascontiguousarray(sd0.verts, F32)
    first, count = n // 4, n // 2
    then = np.array(now, F32, copy=True)
    then[first:first + count] = base[first:first + count]
    put(g, then, first=first, count=count)
    prim2, tv2 = refs_of(g.read_bvh()[1])
    assert np.array_equal(prim2, prim) and np.array_equal(tv2.view(np.uint32), then[prim].view(np.uint32)), f"{label}: the sub-range update reached other slots"
    check_answers(hr, ctx, oracle, g, sd0, _held_step(label + ", then a sub-range", then, prim), label + ", then a sub-range", seed=case + 10)
    g.rebuild_device()
    nodes, tris = check_order(hr, g, then, then[prim], label + ", re-dealt again")
    prim3, _ = refs_of(tris)
    assert int(dc.finite_mask(then)[prim3].sum()) == min(n_refs, int(dc.finite_mask(then).sum())), label
    check_answers(hr, ctx, oracle, g, sd0, _held_step(label + ", re-dealt again", then, prim3), label + ", re-dealt again", seed=case + 20)
    g.close()


def _mesh_ranges(hr, isd):
    """per mesh (first node, node count, first reference, reference count) of the shared deformable scene's arrays"""
    at, ref, out = len(isd.instances), 0, []
    for k, m in enumerate(isd.meshes):
        info = hr.bvh_build_info(m.verts, deformable=bool(sc.FLAGS[k]))
        out.append((at, int(info.n_nodes), ref, int(info.tri_bytes) // 48))
        at += int(info.n_nodes)
        ref += int(info.tri_bytes) // 48
    return out


def _shared_answers(oracle, hr, ctx, g, d, what, seed):
    flat = d.flatten()
    rays = sc.rays(d, d.matrices(), seed=seed)
    gf = hr.Scene(ctx, flat)
    a = answers(g, cuda(rays))
    assert_same(a, answers(gf, cuda(rays)), f"{what}: against the flattened scene")
    assert compare_with_brute_force(g, oracle.Scene(flat), rays, what) == 0
    assert 0.10 <= a[0].mean() <= 0.90, (what, a[0].mean())
    gf.close()


def test_shared_scenes(oracle, hr, ctx):
    """(7) one flagged mesh, both, both in one call against one call each; the unflagged meshes, the top level and the records stand byte for byte"""
    isd = sc.scene()
    d = synth.deform_meshes(isd, 2, {FIELD: "twist", BOX: "wave"}, (FIELD, BOX))
    a, b = [hr.InstancedScene(ctx, isd, shared=True, deformable=sc.FLAGS) for _ in range(2)]
    ranges = _mesh_ranges(hr, isd)
    assert ranges[-1][0] + ranges[-1][1] == len(a.read_bvh()[0])
    for g in (a, b):
        g.update_meshes([entry(d, FIELD), entry(d, BOX)])
    nodes0, tris0 = a.read_bvh()
    rec0 = a.read_records()
    cost0 = a.mesh_refit_cost(FIELD)
    stats0 = a.update_meshes_stats()
    a.rebuild_meshes_device([FIELD])
    assert a.update_meshes_stats() == stats0, "hr_scene_update_meshes_stats counts what the UPDATES enqueued: a re-deal's refit is counted as the re-deal's"
    nodes1, tris1 = a.read_bvh()
    fn, fc, fr, frc = ranges[FIELD]
    assert np.array_equal(nodes1[:fn], nodes0[:fn]) and np.array_equal(nodes1[fn + fc:], nodes0[fn + fc:]), "only the field's nodes change"
    assert np.array_equal(tris1[:fr], tris0[:fr]) and np.array_equal(tris1[fr + frc:], tris0[fr + frc:]) and not np.array_equal(tris1, tris0)
    assert np.array_equal(a.read_records(), rec0)
    prim, tv = refs_of(tris1)
    slots = walk(nodes1, fn)
    assert slots.min() == fr and slots.max() == fr + frc - 1
    order = expected_order(hr, d.meshes[FIELD].verts, d.meshes[FIELD].verts)
    assert np.array_equal(prim[slots], order), "the field's references in Morton order, mesh-local triangle indices"
    _shared_answers(oracle, hr, ctx, a, d, "field re-dealt", 1)
    print(f"shared field: refit cost {cost0:.4f} after the update, {a.mesh_refit_cost(FIELD):.4f} after the re-deal")
    a.rebuild_meshes_device([BOX])
    b.rebuild_meshes_device([BOX, FIELD])
    for x, y, name in zip(a.read_bvh() + (a.read_records(),), b.read_bvh() + (b.read_records(),), ("nodes", "references", "records")):
        assert np.array_equal(x, y), f"one call each against both in one call: {name} differ"
    assert a.mesh_refit_cost(FIELD) == b.mesh_refit_cost(FIELD) and a.mesh_refit_cost(BOX) == b.mesh_refit_cost(BOX)
    nodes2, tris2 = b.read_bvh()
    n_static = ranges[FIELD][0]
    assert np.array_equal(nodes2[:n_static], nodes0[:n_static]) and np.array_equal(tris2[:fr], tris0[:fr]) and np.array_equal(b.read_records(), rec0)
    _shared_answers(oracle, hr, ctx, b, d, "both re-dealt", 2)
    # a sub-range update_meshes over the re-dealt map, then answers again
    d2 = synth.deform_meshes(isd, 3, {FIELD: "wave", BOX: "wave"}, (FIELD, BOX))
    n = d.meshes[FIELD].n_tris
    mixed_field = dc.with_verts(d.meshes[FIELD], d.meshes[FIELD].verts.copy())
    mixed_field.verts[n // 3:n // 3 + n // 4] = d2.meshes[FIELD].verts[n // 3:n // 3 + n // 4]
    mixed = synth.InstancedSceneData(meshes=list(d.meshes[:FIELD]) + [mixed_field, d.meshes[BOX]], instances=list(isd.instances), materials=isd.materials, name="mixed")
    b.update_meshes([entry(mixed, FIELD, first=n // 3, count=n // 4, normals=False)])
    _shared_answers(oracle, hr, ctx, b, mixed, "both re-dealt, then a sub-range update", 3)
    assert a.device_rebuild_counts()["rebuilds_enqueued"] == 2 and b.device_rebuild_counts()["rebuilds_enqueued"] == 2
    a.close(); b.close()


def test_more_meshes_than_one_set_of_launches_takes(oracle, hr, ctx):
    """(7) 70 flagged 12-triangle boxes, more than the 64 meshes one set of launches takes: all in one call (two chunks) against two calls of 35 —
    the same bytes; one re-build counted per mesh; the answers of the flattened scene"""
    base = synth.instanced_cornell(1)
    box = base.meshes[1]
    rng = np.random.RandomState(3)
    M = 70
    meshes = [synth.SceneData(box.verts, box.normals, box.tri_material * 0, box.tri_mesh_id, base.materials, f"box{k}") for k in range(M)]
    inst = [(synth.model_matrix(tuple(float(x) for x in rng.uniform(10, 90, 3)), tuple(rng.uniform(-1, 1, 3)), float(rng.uniform(0, 6.28)), tuple(float(x) for x in rng.uniform(4, 10, 3))), k, 10 + k)
            for k in range(M)]
    isd = synth.InstancedSceneData(meshes=meshes, instances=inst, materials=base.materials, name="seventy_boxes")
    d = synth.deform_meshes(isd, 2, "twist", range(M))
    a, b = [hr.InstancedScene(ctx, isd, shared=True, deformable=[1] * M) for _ in range(2)]
    for g in (a, b):
        g.update_meshes([dict(mesh_idx=k, positions=cuda(d.meshes[k].verts), normals=cuda(d.meshes[k].normals)) for k in range(M)])
    top0, rec0 = a.read_bvh()[0][:M], a.read_records()
    a.rebuild_meshes_device(list(range(M)))
    b.rebuild_meshes_device(list(range(35))); b.rebuild_meshes_device(list(range(35, M)))
    for x, y, name in zip(a.read_bvh() + (a.read_records(),), b.read_bvh() + (b.read_records(),), ("nodes", "references", "records")):
        assert np.array_equal(x, y), f"one call over 70 meshes against two calls: {name} differ"
    assert np.array_equal(a.read_bvh()[0][:M], top0) and np.array_equal(a.read_records(), rec0), "the top level and the records stand"
    assert a.device_rebuild_counts()["rebuilds_enqueued"] == M == b.device_rebuild_counts()["rebuilds_enqueued"]
    prim, _ = refs_of(a.read_bvh()[1])
    assert np.array_equal(np.sort(prim.reshape(M, 12), axis=1), np.tile(np.arange(12), (M, 1))), "every mesh keeps its own twelve triangles"
    flat = d.flatten()
    rays = scene_rays(flat.verts, 8000, 4)
    gf = hr.Scene(ctx, flat)
    ans = answers(a, cuda(rays))
    assert_same(ans, answers(gf, cuda(rays)), "70 meshes re-dealt: against the flattened scene")
    assert compare_with_brute_force(a, oracle.Scene(flat), rays, "70 meshes re-dealt") == 0
    assert 0.10 <= ans[0].mean() <= 0.90, ans[0].mean()
    a.close(); b.close(); gf.close()


def test_errors_enqueue_nothing(hr, ctx):
    """(7) HR_ERR_INVALID_ARG with a message and no launch: an unflagged index, a repeated one, one out of range, n < 0, a scene of another kind"""
    isd = sc.scene()
    g = hr.InstancedScene(ctx, isd, shared=True, deformable=sc.FLAGS)
    flat, plain = hr.Scene(ctx, field(9), deformable=True), hr.Scene(ctx, field(9))
    L = hr.lib()
    for name in ("hr_scene_rebuild_meshes_device", "hr_scene_rebuild_device", "hr_scene_device_rebuild_counts"):
        getattr(L, name).argtypes = hr.DEVICE_REDEAL_ARGTYPES[name]
    g.rebuild_meshes_device([FIELD])
    counts = g.device_rebuild_counts()
    assert counts["rebuilds_enqueued"] == 1 and counts["launches_enqueued"] > 0

    def meshes(h, idx, n=None):
        m = np.asarray(idx, np.uint32)
        return L.hr_scene_rebuild_meshes_device(h, C.c_void_p(m.ctypes.data), len(m) if n is None else n, None)
    for idx, n, what in (([0], None, "not flagged"), ([FIELD, BOX, FIELD], None, "named twice"), ([len(isd.meshes)], None, ">= n_meshes"), ([FIELD], -1, "n < 0")):
        assert meshes(g.h, idx, n) == 1 and "hr_scene_rebuild_meshes_device" in L.hr_last_error().decode() and what in L.hr_last_error().decode(), (idx, L.hr_last_error())
    assert meshes(flat.h, [0]) == 1 and "hr_scene_rebuild_meshes_device" in L.hr_last_error().decode()
    assert g.device_rebuild_counts() == counts and flat.device_rebuild_counts() == dict(rebuilds_enqueued=0, launches_enqueued=0)
    for h in (g.h, plain.h, None):
        assert L.hr_scene_rebuild_device(h, None) == 1 and "hr_scene_rebuild_device" in L.hr_last_error().decode()
    assert g.device_rebuild_counts() == counts
    a, b = C.c_int64(0), C.c_int64(0)
    assert L.hr_scene_device_rebuild_counts(plain.h, C.byref(a), C.byref(b)) == 1
    with pytest.raises(hr.HRError):
        plain.rebuild_device()
    g.rebuild_meshes_device([])
    assert g.device_rebuild_counts() == counts
    g.close(); flat.close(); plain.close()


def test_the_redeal_helps_a_shuffled_cloth(hr, ctx):
    """(8) 4097 triangles, triangle i given the creation vertices of triangle perm(i): the triangle SET is the creation set, only its assignment
    to the leaves is wrong, and that is all a re-deal can mend.  Strictly below the refit's cost; no ratio fixed in advance."""
    sd0 = field(4097)
    perm = np.random.RandomState(7).permutation(sd0.n_tris)
    g = hr.Scene(ctx, sd0, deformable=True)
    g.update_vertices(cuda(sd0.verts[perm]))
    refit = g.refit_cost()
    g.rebuild_device()
    redealt = g.refit_cost()
    g.rebuild()
    print(f"shuffled cloth, 4097 triangles: refit cost {refit:.4f} after the refit, {redealt:.4f} after the device re-deal, {g.refit_cost():.4f} after the host rebuild")
    assert redealt < refit, (redealt, refit)
    g.close()


def test_a_fresh_scene_pays_for_morton_order(hr, ctx):
    """what Morton order costs a tree that had not decayed: re-dealt at its creation vertices the cost is finite and reported, the order is the keys'"""
    sd0 = field(4097)
    g = hr.Scene(ctx, sd0, deformable=True)
    g.rebuild_device()
    cost = g.refit_cost()
    print(f"undecayed field, 4097 triangles: refit cost {cost:.4f} after a device re-deal at the creation vertices")
    assert cost == cost and 0.0 < cost < float("inf")
    check_order(hr, g, sd0.verts, sd0.verts, "creation vertices")
    g.close()


def test_counters_and_a_stream_ordered_sequence(oracle, hr, ctx):
    """(9) one re-build per mesh; the second call enqueues what the first did (nothing is allocated late or skipped); update -> re-deal -> trace on
    one stream without a host synchronisation between them"""
    import torch
    for n in (4096, 4097):
        g = hr.Scene(ctx, field(n), deformable=True)
        assert g.device_rebuild_counts() == dict(rebuilds_enqueued=0, launches_enqueued=0)
        g.rebuild_device()
        c1 = g.device_rebuild_counts()
        g.rebuild_device()
        c2 = g.device_rebuild_counts()
        assert c1["rebuilds_enqueued"] == 1 and c2["rebuilds_enqueued"] == 2 and c2["launches_enqueued"] == 2 * c1["launches_enqueued"], (n, c1, c2)
        # bounds + the sort (1, or keys + 4 x 3) + gather + commit, then the refit's launches (its bounds among them)
        assert c1["launches_enqueued"] >= (4 if n <= 4096 else 16) + 2, (n, c1)
        g.close()
    sd0 = field(8192)
    sd = synth.deform(sd0, 3, "twist")
    g, gf, osc = hr.Scene(ctx, sd0, deformable=True), hr.Scene(ctx, sd), oracle.Scene(sd)
    rays = rc.edge_and_vertex_rays(sd.verts, seed=3, max_tris=150)
    pos, nrm, rd = cuda(sd.verts), cuda(sd.normals), cuda(rays)
    torch.cuda.synchronize()
    # torch's current stream, not a stream of its own: torch makes its whole stream pool with the first torch.cuda.Stream() of a process, and that
    # pool then stands beside every later test's streams and graphs for the rest of the session
    g.update_vertices(pos, nrm)
    g.rebuild_device()
    occ = g.any_hit(rd)
    tuv, prim = g.closest_hit(rd)
    a = (occ.cpu().numpy(), tuv.cpu().numpy(), prim.cpu().numpy())       # the first wait of the sequence
    assert_same(a, answers(gf, rd), "update -> re-deal -> trace on one stream")
    assert compare_with_brute_force(g, osc, rays, "stream-ordered") == 0
    assert 0.10 <= a[0].mean() <= 0.90
    g.close(); gf.close()
