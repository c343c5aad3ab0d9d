"""The adversarial ray sets of tests/ray_cases.py, checked without a GPU: the INPUTS are what they claim to be (on the planes, to either
side of them, balanced between hits and misses) and the REFERENCE is sound (the oracle's brute-force path leaks through no shared edge or
vertex, and its BVH2 walk agrees with it bit for bit) before tests/test_gpu_ray_edges.py compares the HIP traversal with either."""
import numpy as np
import pytest

import helpers
import ray_cases as rc

SCENES = ("cornell", "sponza_small", "chain", "soup_sheets", "soup_grid")
MAX_BOXES = 400


def scene_verts(name):
    """(float32 [n][3][3], build switches)"""
    if name == "chain":
        from test_gpu_trace import _chain_scene
        return _chain_scene().verts, {}
    if name.startswith("soup_"):
        return rc.soup_of_kind(name[5:], seed=11)
    return helpers.scene_data(name).verts, {}


def scene_data_of(name):
    from hybrid_rendering_amd import synth
    v, env = scene_verts(name)
    if not name.startswith("soup_") and name != "chain":
        return helpers.scene_data(name), env
    return synth.SceneData(v, np.zeros_like(v), np.zeros(len(v), np.uint32), np.ones(len(v), np.uint32), np.array([[0.5] * 3 + [0, 0.5, 0, 0, 0]], np.float32), name), env


def sampled_boxes(verts, seed=0, max_boxes=MAX_BOXES):
    """child boxes of the product's BVH over `verts`, sampled evenly over the depths when there are more than max_boxes"""
    from hybrid_rendering_amd import api
    boxes = api.bvh_child_boxes(verts)
    if len(boxes) <= max_boxes:
        return boxes
    rng = np.random.RandomState(seed)
    depths = np.unique(boxes["depth"])
    per = max(1, max_boxes // len(depths))
    pick = np.concatenate([rng.permutation(np.flatnonzero(boxes["depth"] == d))[:per] for d in depths])
    return boxes[np.sort(pick)]


def generated_sets(name, verts):
    """{generator: rays} for a scene, as both test files draw them"""
    boxes = sampled_boxes(verts)
    return {"edge_and_vertex": rc.edge_and_vertex_rays(verts, seed=1), "box_grazers": rc.box_grazers(boxes, seed=2), "far_origin": rc.far_origin_rays(verts, seed=3)}


def check_rays(rays):
    assert rays.dtype == np.float32 and rays.ndim == 2 and rays.shape[1] == 8 and len(rays) > 0
    assert np.isfinite(rays[:, [0, 1, 2, 4, 5, 6, 7]]).all()
    tm = rays[:, 3]
    assert (np.isfinite(tm) | (tm == np.inf)).all() and (tm >= 0).all()
    n = np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1)
    assert np.abs(n - 1.0).max() <= 2 * np.finfo(np.float32).eps, np.abs(n - 1.0).max()


def test_child_boxes_export_matches_the_builder():
    """hr_bvh_child_boxes: one record per non-empty child slot; the root's children together bound the scene; depths and leaf flags are
    consistent with hr_bvh_build_info"""
    from hybrid_rendering_amd import api
    for name in ("cornell", "sponza_small"):
        v, _ = scene_verts(name)
        boxes, info = api.bvh_child_boxes(v), api.bvh_build_info(v)
        assert boxes["node"].max() == info.n_nodes - 1 and boxes["depth"].max() == info.max_depth - 1 or boxes["depth"].max() == info.max_depth
        assert (boxes["lo"] <= boxes["hi"]).all() and (boxes["step"] > 0).all()
        root = boxes[boxes["node"] == 0]
        p = v.reshape(-1, 3)
        assert (root["lo"].min(0) <= p.min(0)).all() and (root["hi"].max(0) >= p.max(0)).all()
        assert boxes["is_leaf"].sum() > 0 and len(np.unique(boxes[["node", "slot"]])) == len(boxes)
        # every triangle lies in at least one leaf box entirely or in part: its centroid is inside some leaf box
        leaves = boxes[boxes["is_leaf"] == 1]
        c = v.mean(1)[:200]
        inside = ((c[:, None, :] >= leaves["lo"][None]) & (c[:, None, :] <= leaves["hi"][None])).all(2).any(1)
        assert inside.all()


@pytest.mark.parametrize("name", SCENES)
def test_generators_shape_determinism_units(name):
    v, _ = scene_verts(name)
    a, b = generated_sets(name, v), generated_sets(name, v)
    for k in a:
        check_rays(a[k])
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert not np.array_equal(rc.edge_and_vertex_rays(v, seed=1)[:64], rc.edge_and_vertex_rays(v, seed=5)[:64])
    kn, m = rc.interval_knife_edges(a["edge_and_vertex"][:100], np.linspace(-1, 5, 100).astype(np.float32), meta=True)
    check_rays(kn)
    assert len(kn) == 10 * int((np.linspace(-1, 5, 100) > 0).sum()) and (m[:, 1] == np.tile(np.arange(10), len(kn) // 10)).all()
    t = np.float32(1.5)
    one = rc.interval_knife_edges(a["edge_and_vertex"][:1], [t])
    assert one[0, 3] == np.nextafter(t, np.float32(0)) and one[1, 3] == t and one[2, 3] == np.nextafter(t, np.float32(2))
    assert one[3, 7] == np.nextafter(t, np.float32(0)) and one[4, 7] == t and one[5, 7] == np.nextafter(t, np.float32(2)) and (one[3:6, 3] == np.inf).all()
    assert one[6, 3] == one[6, 7] == t and one[7, 3] == 0 and one[8, 3] == np.inf and one[9, 3] == rc.FLT_MAX


def test_step_ulps_and_lerp_are_exact():
    x = np.float32([1.0, -1.0, 0.0, 3.5e10, 1e-30])
    assert np.array_equal(rc.step_ulps(x, 1), np.nextafter(x, np.float32(np.inf)))
    assert np.array_equal(rc.step_ulps(x, -2), np.nextafter(np.nextafter(x, np.float32(-np.inf)), np.float32(-np.inf)))
    assert np.array_equal(rc.step_ulps(rc.step_ulps(x, 8), -8), x)
    a, b = np.float32([[1, 2, 3]]), np.float32([[4, 6, 8]])
    assert np.array_equal(rc.lerp32(a, b, [0.0]), a) and np.array_equal(rc.lerp32(a, b, [1.0]), b) and np.array_equal(rc.lerp32(a, b, [0.5]), np.float32([[2.5, 4, 5.5]]))


def test_far_origins_are_as_far_as_they_say():
    v, _ = scene_verts("cornell")
    rays, fi = rc.far_origin_rays(v, meta=True)
    lo, hi, diag = rc.scene_box(v)
    dist = np.linalg.norm(rays[:, :3].astype(np.float64) - (lo + hi) * 0.5, axis=1) / diag
    for k, f in enumerate(rc.FAR_FACTORS):
        assert (fi == k).sum() > 100 and np.allclose(dist[fi == k], f, rtol=1e-5)


def test_box_grazers_lie_on_both_sides_of_every_face_of_the_cornell_boxes():
    """float64 check against the boxes: for every box and face the set holds rays that run in the plane itself, strictly on its outer side
    and strictly on its inner side (origin coordinate != plane, direction component exactly 0), and rays through it"""
    from hybrid_rendering_amd import api
    v, _ = scene_verts("cornell")
    boxes = api.bvh_child_boxes(v)
    rays, meta = rc.box_grazers(boxes, seed=2, meta=True)
    o, d = rays[:, :3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    for b in range(len(boxes)):
        for face in range(6):
            ax, side = face // 2, face % 2
            plane = float((boxes["hi"] if side else boxes["lo"])[b, ax])
            sel = (meta[:, 0] == b) & (meta[:, 1] == face) & (d[:, ax] == 0.0)
            rel = o[sel, ax] - plane
            assert (rel == 0).any() and (rel < 0).any() and (rel > 0).any(), (b, face)
            ulp = float(np.spacing(np.float32(abs(plane))))
            assert (np.abs(rel[rel != 0]).min() <= ulp) and np.abs(rel).max() >= float(boxes["step"][b, ax]) * 0.999, (b, face)
            for kind in range(4):
                assert ((meta[:, 0] == b) & (meta[:, 1] == face) & (meta[:, 2] == kind)).sum() >= 5
            tiny = (meta[:, 0] == b) & (meta[:, 1] == face) & (d[:, ax] != 0) & (np.abs(d[:, ax]) < 1e-18)
            assert tiny.any(), (b, face)
    # along-edge rays: an exact axis direction and two coordinates on (stepped) box planes
    e = meta[:, 2] == 2
    assert (np.abs(d[e]).sum(1) == 1.0).all() and (np.abs(d[e]).max(1) == 1.0).all()


def _facing_margin_ok(V, F, rays, margin=0.05):
    """float64 re-check of the premise of watertight_rays on the finished rays: the ray's line meets the solid — the nearest point of entry is
    on a face that faces the origin by the margin"""
    Vd = V.astype(np.float64)
    n = np.cross(Vd[F[:, 1]] - Vd[F[:, 0]], Vd[F[:, 2]] - Vd[F[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h = (n * Vd[F[:, 0]]).sum(1)
    o, d = rays[:, :3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    # convex solid = intersection of half spaces n.x <= h: the line's parameter interval inside it (slab clipping, float64)
    dn, on = d @ n.T, o @ n.T - h
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -on / dn
    t_in = np.where(dn < 0, t, -np.inf).max(1)
    t_out = np.where(dn > 0, t, np.inf).min(1)
    return (t_out - t_in) / np.maximum(np.abs(t_in), 1e-300), t_in


def test_brute_force_oracle_is_watertight_on_closed_convex_meshes(oracle):
    """icospheres (1-3 subdivisions), a cube and a tetrahedron under random rotations at scales 1e-3 .. 1e3: a ray with t_max = +inf from an
    outside origin through a point of a non-silhouette edge, or through a vertex whose faces all face the origin, enters the solid — the
    brute-force any-hit and closest-hit queries must report a hit.  Leaks allowed: 0."""
    total = 0
    for k, (name, V, F) in enumerate(rc.closed_meshes(seed=4)):
        rays = rc.watertight_rays(V, F, seed=100 + k)
        check_rays(rays)
        assert len(rays) >= (300 if name.startswith("ico") else 20), (name, len(rays))
        depth, t_in = _facing_margin_ok(V, F, rays)
        assert (depth > 1e-6).all() and (t_in > 0).all(), f"{name}: a ray of the set does not cross the solid in float64 ({int((depth <= 1e-6).sum())})"
        tris = rc.mesh_triangles(V, F)
        sd, _ = _sd(tris, name)
        osc = oracle.Scene(sd)
        occ = osc.any_hit(rays, brute_force=True)
        tuv, prim = osc.closest_hit(rays, brute_force=True)
        leaks = np.flatnonzero((occ == 0) | (prim < 0))
        assert len(leaks) == 0, f"{name}: {len(leaks)} of {len(rays)} rays leak through the closed mesh; first: {[[float(x).hex() for x in rays[i]] for i in leaks[:3]]}"
        assert np.array_equal(occ, osc.any_hit(rays)) and np.array_equal(prim, osc.closest_hit(rays)[1])
        total += len(rays)
    assert total > 15000


def _sd(tris, name):
    from hybrid_rendering_amd import synth
    return synth.SceneData(tris, np.zeros_like(tris), np.zeros(len(tris), np.uint32), np.ones(len(tris), np.uint32), np.array([[0.5] * 3 + [0, 0.5, 0, 0, 0]], np.float32), name), {}


def assert_oracle_paths_agree(osc, rays, what):
    """brute force == BVH2 walk: flags, primitive, and t, u, v bit for bit; returns the brute-force answers"""
    occ, occ2 = osc.any_hit(rays, brute_force=True), osc.any_hit(rays)
    (tuv, prim), (tuv2, prim2) = osc.closest_hit(rays, brute_force=True), osc.closest_hit(rays)
    assert np.array_equal(occ != 0, occ2 != 0), f"{what}: the oracle's any-hit paths differ on {int(((occ != 0) != (occ2 != 0)).sum())} rays"
    assert np.array_equal(prim, prim2), f"{what}: the oracle's closest-hit paths differ on {int((prim != prim2).sum())} rays"
    hit = prim >= 0
    assert np.array_equal(tuv[hit].view(np.uint32), tuv2[hit].view(np.uint32)), f"{what}: t, u, v differ between the oracle's paths"
    return occ, tuv, prim


@pytest.mark.parametrize("name", SCENES)
def test_reference_paths_agree_and_sets_are_balanced(oracle, name):
    """per generator and scene: the oracle's brute-force and BVH2 answers are the same bits, and the brute-force hit fraction lies in
    [0.10, 0.90] — a set nearly all hits or all misses would let a broken walk pass"""
    sd, _ = scene_data_of(name)
    osc = oracle.Scene(sd)
    for gen, rays in generated_sets(name, sd.verts).items():
        occ, tuv, prim = assert_oracle_paths_agree(osc, rays, f"{name}/{gen}")
        frac = float((occ != 0).mean())
        print(f"{name}/{gen}: {len(rays)} rays, brute-force hit fraction {frac:.3f}")
        assert 0.10 <= frac <= 0.90, (name, gen, frac)


@pytest.mark.parametrize("name", ("cornell", "sponza_small"))
def test_knife_edges_flip_the_answer(oracle, name):
    """interval_knife_edges from the oracle's closest hits: t_max one ulp before / behind the hit distance must flip the any-hit answer, t_min
    one ulp before / behind it the closest primitive, for at least 25 % of the rays each; both oracle paths agree on all copies"""
    sd, _ = scene_data_of(name)
    osc = oracle.Scene(sd)
    base = rc.edge_and_vertex_rays(sd.verts, seed=7, t_max="inf")[:4000]
    tuv, prim = osc.closest_hit(base, brute_force=True)
    kn = rc.interval_knife_edges(base, np.where(prim >= 0, tuv[:, 0], np.nan))
    check_rays(kn)
    occ, ktuv, kprim = assert_oracle_paths_agree(osc, kn, f"{name}/knife")
    A, P = (occ != 0).reshape(-1, 10), kprim.reshape(-1, 10)
    flip_max, flip_min = float((A[:, 0] != A[:, 2]).mean()), float((P[:, 3] != P[:, 5]).mean())
    print(f"{name}: {len(kn)} knife-edge rays, hit fraction {A.mean():.3f}, t_max flips {flip_max:.3f}, t_min flips {flip_min:.3f}")
    assert flip_max >= 0.25 and flip_min >= 0.25
    assert 0.10 <= A.mean() <= 0.90
    assert not A[:, 6].any() and not A[:, 7].any(), "an empty interval (t_min == t_max, t_max == 0) holds no hit"
    assert np.array_equal(A[:, 8], A[:, 9]) and A[:, 8].all()


def test_soup_moved_not_changed():
    """the soups the tool drew before the move: same stream of RandomState(0) -> same kinds and sizes (pins the draw order)"""
    rng = np.random.RandomState(0)
    seen = []
    for _ in range(6):
        k, v = rc.soup(rng)
        seen.append((k, len(v)))
        rng.randint(len(rc.SWITCHES))
    assert all(k in rc.SOUP_KINDS for k, _ in seen) and all(v.dtype == np.float32 for v in [rc.soup(np.random.RandomState(1))[1]])
    import importlib.util, os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_bvh.py")).read()
    assert "from ray_cases import soup, SWITCHES" in src and "def soup(" not in src
