"""The HIP BVH walk against BRUTE FORCE at its edges (tests/ray_cases.py): rays in the face planes of the child boxes, along their edges and
through their corners, an ulp and a quantisation step to either side; rays through triangle edges and vertices; t_max / t_min one ulp
around a hit; origins up to 1e6 scene diagonals away; the fuzzer's soups; instanced scenes after updates, and updates enqueued back to back.

Reference everywhere: the oracle's brute-force queries (no box test of any kind).  Compared: any-hit flags, closest-hit primitive, and
t, u, v as bit patterns.  Mismatches allowed: 0.  The box test of the walk (traverse.h test_node) only has to be conservative; its error
budget is DESIGN.md section 3.3 — these tests are what holds a change of ray_prepare / test_node / the box pad to it.

Not covered here, but in tests/test_gpu_trace_gbuffer_edges.py: the shadow and AO passes' own trace kernels (ray set-up from the G-buffer,
fire / no-fire decisions, edge threads, the occluder cache's per-lane triangle test, the AO entry-node table) on synthesised G-buffers
whose pixel rays run through triangle edges, vertices and box planes — pinned to the same brute force.
The two closest-hit launches (k_ddgi_trace, k_refl_trace) and the probe update: tests/test_gpu_closest_edges.py, tests/test_gpu_probe_update_edges.py."""
import numpy as np
import pytest

import ray_cases as rc
from test_ray_cases import scene_data_of, sampled_boxes, _sd

pytestmark = pytest.mark.gpu

BUILDS = {"default": {}, "split": {"HR_BVH_SPLIT": "0.1"}, "sah3": {"HR_BVH_SAH_DEPTH": "3"}}
SCENES = ("cornell", "sponza_small", "chain", "soup_sheets", "soup_grid")


def set_build_env(monkeypatch, env):
    import os
    for k in list(os.environ):
        if k.startswith("HR_BVH_"):
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def hexrow(r):
    return " ".join(float(x).hex() for x in r)


def gpu_answers(gsc, rays):
    import torch
    rd = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    occ = gsc.any_hit(rd).cpu().numpy()
    gt, gp = gsc.closest_hit(rd)
    return occ, gt.cpu().numpy(), gp.cpu().numpy()


def compare_with_brute_force(gsc, osc, rays, what, describe=None):
    """0 mismatches between the HIP queries and the oracle's brute force; returns (occluded, tuv, prim) of the reference"""
    ref_occ = osc.any_hit(rays, brute_force=True)
    ref_tuv, ref_prim = osc.closest_hit(rays, brute_force=True)
    occ, tuv, prim = gpu_answers(gsc, rays)
    hit = ref_prim >= 0
    bad_any = (ref_occ != 0) != (occ != 0)
    bad_prim = ref_prim != prim
    bad_tuv = hit & (prim >= 0) & (ref_tuv.view(np.uint32) != tuv.view(np.uint32)).any(1)
    bad = bad_any | bad_prim | bad_tuv
    print(f"{what}: {len(rays)} rays, hit fraction {float((ref_occ != 0).mean()):.3f}; mismatches any-hit {int(bad_any.sum())}, primitive {int(bad_prim.sum())}, t/u/v {int(bad_tuv.sum())}")
    if bad.any():
        lines = []
        for i in np.flatnonzero(bad)[:6]:
            lines.append(f"  ray {i}: {hexrow(rays[i])}\n    any-hit ref {int(ref_occ[i])} got {int(occ[i])}; closest ref prim {int(ref_prim[i])} t,u,v {hexrow(ref_tuv[i])}; got prim {int(prim[i])} t,u,v {hexrow(tuv[i])}"
                         + (("\n    " + describe(i)) if describe else ""))
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(rays)} rays differ from brute force (any-hit {int(bad_any.sum())}, primitive {int(bad_prim.sum())}, t/u/v {int(bad_tuv.sum())})\n" + "\n".join(lines))
    return ref_occ, ref_tuv, ref_prim


def perm_code(rays):
    """traverse.h perm_code of each ray: kz * 2 + (direction negative along kz)"""
    d = rays[:, 4:7]
    a = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    kz[a[:, 1] > a[:, 0]] = 1
    kz[a[:, 2] > np.where(kz == 0, a[:, 0], a[:, 1])] = 2
    return kz * 2 + (d[np.arange(len(d)), kz] < 0)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", SCENES)
def test_box_grazers_match_brute_force(oracle, hr, ctx, monkeypatch, name, build):
    """rays in, beside and through the faces, edges and corners of the child boxes the traversal tests (sampled over every depth)"""
    sd, env = scene_data_of(name)
    set_build_env(monkeypatch, {**env, **BUILDS[build]})
    boxes = sampled_boxes(sd.verts)
    rays, meta = rc.box_grazers(boxes, seed=2, meta=True)
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)

    def describe(i):
        b = boxes[meta[i, 0]]
        return (f"aimed at node {int(b['node'])} slot {int(b['slot'])} (depth {int(b['depth'])}, {'leaf' if b['is_leaf'] else 'internal'}), face axis {meta[i, 1] // 2} "
                f"{'hi' if meta[i, 1] % 2 else 'lo'}, {rc.GRAZE_KINDS[meta[i, 2]]}; box lo {hexrow(b['lo'])} hi {hexrow(b['hi'])} step {hexrow(b['step'])}")
    try:
        compare_with_brute_force(gsc, osc, rays, f"{name}/{build}/box_grazers", describe)
    finally:
        gsc.close()


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", SCENES)
def test_edge_and_vertex_rays_match_brute_force(oracle, hr, ctx, monkeypatch, name, build):
    """rays through points exactly on triangle edges and vertices (and 1, 2, 8 ulps off), submitted twice: sorted by permutation code (the
    waves take ray_tri_raw_uniform's constant-folded path) and interleaved (mixed waves) — identical answers per ray, equal to brute force"""
    sd, env = scene_data_of(name)
    set_build_env(monkeypatch, {**env, **BUILDS[build]})
    rays, tri = rc.edge_and_vertex_rays(sd.verts, seed=1, meta=True)
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
    try:
        code = perm_code(rays)
        by_code = np.argsort(code, kind="stable")
        assert len(np.unique(code)) == 6
        # interleaved: neighbouring lanes hold different codes wherever the set allows it
        rank = np.zeros(len(rays), np.int64)
        for c in range(6):
            rank[code == c] = np.arange(int((code == c).sum()))
        mixed = np.lexsort((code, rank))
        assert (np.diff(code[by_code]) != 0).sum() == 5 and (np.diff(code[mixed][: 6 * int(np.bincount(code).min())]) != 0).all()
        describe = lambda order: (lambda i: f"aimed at triangle {int(tri[order[i]])}, perm_code {int(code[order[i]])}")
        compare_with_brute_force(gsc, osc, rays[by_code], f"{name}/{build}/edge_and_vertex sorted by perm_code", describe(by_code))
        compare_with_brute_force(gsc, osc, rays[mixed], f"{name}/{build}/edge_and_vertex interleaved", describe(mixed))
        a, b = gpu_answers(gsc, rays[by_code]), gpu_answers(gsc, rays[mixed])
        inv_a, inv_b = np.argsort(by_code), np.argsort(mixed)
        for x, y in zip(a, b):
            assert np.array_equal(x[inv_a].view(np.uint8 if x.dtype == np.uint8 else np.uint32), y[inv_b].view(np.uint8 if y.dtype == np.uint8 else np.uint32)), "uniform and mixed waves answer differently"
    finally:
        gsc.close()


def test_closed_meshes_are_watertight_on_the_gpu(oracle, hr, ctx):
    """the closed convex meshes of tests/test_ray_cases.py: rays through non-silhouette edges and vertices must hit (any-hit and closest hit)
    on the GPU as they do for the brute-force oracle.  Leaks allowed: 0."""
    total = 0
    for k, (name, V, F) in enumerate(rc.closed_meshes(seed=4)):
        rays = rc.watertight_rays(V, F, seed=100 + k)
        sd, _ = _sd(rc.mesh_triangles(V, F), name)
        osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
        try:
            compare_with_brute_force(gsc, osc, rays, f"watertight/{name}")
            occ, tuv, prim = gpu_answers(gsc, rays)
            leaks = np.flatnonzero((occ == 0) | (prim < 0))
            assert len(leaks) == 0, f"{name}: {len(leaks)} of {len(rays)} rays leak through the closed mesh on the GPU; first: {[hexrow(rays[i]) for i in leaks[:3]]}"
        finally:
            gsc.close()
        total += len(rays)
    assert total > 15000


@pytest.mark.parametrize("name", ("cornell", "sponza_small"))
def test_interval_knife_edges_match_brute_force(oracle, hr, ctx, name):
    """t_max and t_min one ulp before / at / behind the oracle's closest-hit distance, and the empty and unbounded intervals"""
    sd, _ = scene_data_of(name)
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
    try:
        for seed, gen in ((7, "edge"), (8, "grazer")):
            base = rc.edge_and_vertex_rays(sd.verts, seed=seed, t_max="inf")[:6000] if gen == "edge" else rc.box_grazers(sampled_boxes(sd.verts), seed=seed, t_max="inf")[:6000]
            tuv, prim = osc.closest_hit(base, brute_force=True)
            kn, m = rc.interval_knife_edges(base, np.where(prim >= 0, tuv[:, 0], np.nan), meta=True)
            occ, _, _ = compare_with_brute_force(gsc, osc, kn, f"{name}/knife edges from {gen} rays", lambda i: f"copy {rc.KNIFE_KINDS[m[i, 1]]} of base ray {int(m[i, 0])}")
            A = (occ != 0).reshape(-1, 10)
            assert (A[:, 0] != A[:, 2]).mean() >= 0.25
    finally:
        gsc.close()


SOUP_SEEDS = (1000, 1001, 1003, 1004, 1005, 1006, 1007, 1009, 1011, 1013, 1015, 1016, 1017, 1018, 1019, 1020, 1021, 1022, 1027, 1029, 1030, 1032, 1033, 1034, 1035, 1036, 1037, 1038,
              1040, 1041, 1043, 1044, 1049, 1050, 1053, 1060, 1061, 1062, 1070, 1080)


def test_fuzzer_soups_match_brute_force(oracle, hr, ctx, monkeypatch):
    """40 fixed seeds of the fuzzer's soups (tools/fuzz_bvh.py draws from the same generator; five of each kind, at most 13 k triangles) with the
    build switches the tool draws for them; its random + aimed rays plus rays through edges and vertices.  Coincident duplicates (equal t)
    resolve to the smallest primitive index on both sides."""
    kinds = {}
    for seed in SOUP_SEEDS:
        rng = np.random.RandomState(seed)
        kind, v = rc.soup(rng)
        env = dict(rc.SWITCHES[int(rng.randint(len(rc.SWITCHES)))])
        assert len(v) <= 13000
        kinds[kind] = kinds.get(kind, 0) + 1
        set_build_env(monkeypatch, env)
        sd, _ = _sd(v, f"soup{seed}")
        osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
        try:
            rays = np.concatenate([rc.soup_rays(rng, v, 12000), rc.edge_and_vertex_rays(v, seed=seed, max_tris=60)])
            ref_occ, ref_tuv, ref_prim = compare_with_brute_force(gsc, osc, rays, f"soup seed {seed}: {kind}, {len(v)} triangles, {env}")
            # ties: the first of a group of identical triangles is the one reported
            _, first, inverse = np.unique(v.reshape(len(v), 9).view(np.uint32), axis=0, return_index=True, return_inverse=True)
            canon = np.asarray(first)[np.asarray(inverse).reshape(-1)]
            _, _, prim = gpu_answers(gsc, rays)
            hit = ref_prim >= 0
            assert np.array_equal(canon[ref_prim[hit]], ref_prim[hit]) and np.array_equal(canon[prim[hit]], prim[hit]), "a duplicate with a larger index was reported"
            if kind == "dupes":
                assert (canon != np.arange(len(v))).sum() > 0 and hit.any()
        finally:
            gsc.close()
    assert len(kinds) == len(rc.SOUP_KINDS) and min(kinds.values()) >= 3, kinds


@pytest.mark.parametrize("factor", rc.FAR_FACTORS)
@pytest.mark.parametrize("name", ("cornell", "sponza_small"))
def test_far_origins_match_brute_force(oracle, hr, ctx, name, factor):
    """origins `factor` scene diagonals from the scene's centre, aimed at edge points, vertices and centroids, generic and near-axis.
    Measured on an MI355X: 0 mismatches at every factor up to 1e6 (the box test's margins are relative), so no
    origin domain has to be stated; with the box pad and the far-plane scale removed the same rays differ on 13-32 of 512 (cornell) and
    6-1076 of 4800 (sponza_small, growing with the factor)."""
    sd, _ = scene_data_of(name)
    rays = rc.far_origin_rays(sd.verts, factors=(factor,), seed=3, max_tris=300)
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
    try:
        compare_with_brute_force(gsc, osc, rays, f"{name}/far origins x{factor:g}")
    finally:
        gsc.close()


def _instanced(n_boxes=70, seed=9):
    from hybrid_rendering_amd import synth
    return synth.instanced_cornell(n_boxes, seed=seed)


def test_instanced_scene_after_updates_matches_brute_force(oracle, hr, ctx):
    """71 instances, three updates (every second instance moves and rotates): edge / vertex rays and far origins (1 and 10 diagonals) against
    brute force over the flattened, transformed triangles"""
    from test_gpu_instances import _mats
    n_boxes, seed = 70, 9
    isd = _instanced(n_boxes, seed)
    g = hr.InstancedScene(ctx, isd)
    try:
        for f in (1, 2, 7):
            mats = _mats(isd, n_boxes, seed, f)
            g.update(mats)
        flat = isd.flatten(mats)
        osc = oracle.Scene(flat)
        compare_with_brute_force(g, osc, rc.edge_and_vertex_rays(flat.verts, seed=1), "instanced/edge_and_vertex")
        compare_with_brute_force(g, osc, rc.far_origin_rays(flat.verts, factors=(1.0, 10.0), seed=3, max_tris=300), "instanced/far origins x1, x10")
    finally:
        g.close()


def test_back_to_back_instance_updates_take_effect_in_order(oracle, hr, ctx):
    """One stream: a batch of 1080p G-buffer raycasts, then 8 hr_scene_update_instances calls with different matrices — one of them with the
    matrices of the call before it (the nothing-moved early return) — with NO host synchronisation in between, then the queries.  The
    answers are those of a fresh scene created at the final matrices, and of brute force over the flattened triangles.  (Regression test
    of the staged uploads in instances.hip: the host mirrors the asynchronous copies read are not rewritten while a copy is pending.)"""
    import torch
    from hybrid_rendering_amd import synth
    from test_gpu_instances import _mats, _rays
    import helpers
    n_boxes, seed = 70, 9
    isd = _instanced(n_boxes, seed)
    g = hr.InstancedScene(ctx, isd)
    frames = (1, 2, 3, 3, 40, 41, 90, 91)
    all_mats = [_mats(isd, n_boxes, seed, f) for f in frames]
    assert np.array_equal(all_mats[2], all_mats[3]) and not np.array_equal(all_mats[-1], all_mats[-2])
    flat = isd.flatten(all_mats[-1])
    rays = np.concatenate([_rays(40000, seed), rc.edge_and_vertex_rays(flat.verts, seed=1, max_tris=150)])
    rd = torch.from_numpy(rays).cuda()
    W, H = 1920, 1080
    ubo = synth.make_ubo(helpers.cameras("cornell", W / H, 1, 0.0)[0], None, helpers.light_for("cornell"))
    torch.cuda.synchronize()
    try:
        keep = [g.gbuffer(ubo, W, H) for _ in range(12)]   # ordinary work the updates queue up behind
        for m in all_mats:
            g.update(m)
        occ, (tuv, prim) = g.any_hit(rd), g.closest_hit(rd)
        torch.cuda.synchronize()
        occ, tuv, prim = occ.cpu().numpy(), tuv.cpu().numpy(), prim.cpu().numpy()
        fresh = hr.InstancedScene(ctx, synth.InstancedSceneData(isd.meshes, synth.instanced_cornell_instances(n_boxes, seed=seed, frame=frames[-1]), isd.materials))
        try:
            f_occ, f_tuv, f_prim = gpu_answers(fresh, rays)
        finally:
            fresh.close()
        assert np.array_equal(occ, f_occ), f"any-hit differs from a fresh scene at the final matrices on {int((occ != f_occ).sum())} rays"
        assert np.array_equal(prim, f_prim) and np.array_equal(tuv.view(np.uint32), f_tuv.view(np.uint32)), f"closest hits differ from a fresh scene on {int((prim != f_prim).sum())} rays"
        compare_with_brute_force(g, oracle.Scene(flat), rays, "back-to-back updates")
        assert 0.05 < (occ != 0).mean() < 0.999
        del keep
    finally:
        g.close()
