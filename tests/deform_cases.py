"""Hostile vertex streams for the deformable scenes (hr_scene_update_vertices / hr_scene_update_meshes): what a simulation hands the refit when it
starts from a placeholder, blows up, collapses, drifts away or goes non-finite.  tests/test_deform_cases.py checks with the oracle alone that the
streams can tell a right answer from a wrong one; tests/test_gpu_deform_edges.py walks one live scene through each of them.

A stream is a list of Step(label, verts, kind): `verts` a full [n][3][3] float32 array with the creation topology, step 0 what the scene is created
from.  kind: "finite" (every triangle finite, the reference hits a fair share of every ray set), "nothing" (the reference hits nothing by
construction: no finite triangle, or every triangle without area) and "poisoned" (some triangles non-finite; Step.poisoned lists them).

Families (the scale ladders run about the centre of the base's box, computed in double and rounded once):
  grow       creation from a placeholder — "point": every vertex the base's first vertex; "seed": the base scaled by 2^-18 (see below) — then the
             base, the base inflated by 2^4, 2^8, 2^12, 2^30, and the base again
  shrink     2^-12, 2^-30, one axis flattened to exactly zero extent (a plane), two axes (a line), one point, the base again
  drift      the base translated by 5000, 50000, 8190 (trace_cases.FAR_OFFSETS' places) and 2^20 on one axis, then on all three, the base again
  nonfinite  (a) one coordinate of one vertex -inf / +inf / NaN on each axis, (b) a whole triangle NaN, (c) every triangle of one leaf non-finite,
             (d) a random 30 % of the triangles with one random +-inf / NaN coordinate each, (e) every triangle non-finite; the base after each

Where the reference degenerates.  The bases live around (50, 50, 50), where a float32 step is 3.8e-6.
  * The 2^-30 rung (extent 1e-7) snaps every vertex onto ONE float: it is "nothing", like "point".  A line's triangles have no area (the
    watertight test's determinant is exactly 0 for every ray), so "line" is "nothing" too.
  * The seed placeholder is 2^-18, not 2^-20: the last rung at which the reference's hits lie ON their triangles.  At 2^-20 the heightfield is a
    lattice of 25 x 4 x 25 floats; rays that run along box faces then lie exactly IN the plane of sliver triangles, all three edge functions
    of the fp32 watertight test are rounding noise, and where their signs happen to agree brute force reports a hit up to 9.5 float steps
    (3.6e-5, a third of the scene, 1.5 leaf pads) away from the triangle it names — 4 of 43 577 rays, measured with hit_offsets() below; no
    box pad can follow an arbitrary one.  From 2^-18 up (extent 100 float steps) every hit of every set lies within a thousandth of the
    pad of its triangle; tests/test_deform_cases.py asserts at most HALF the pad of DESIGN.md section 3.3 for every step of every stream
    (the other half is the box test's own).
  * 2^30 stays far from fp32 overflow (products of the watertight test reach 1e33), so the ladders are not shortened at their upper end."""
from collections import namedtuple

import numpy as np

import ray_cases as rc
from hybrid_rendering_amd import synth
from test_gpu_deformable import sample

F32 = np.float32
Step = namedtuple("Step", "label verts kind poisoned")
FAMILIES = ("grow_point", "grow_seed", "shrink", "drift", "nonfinite")
BASES = {"heightfield16": lambda: synth.heightfield(16), "cornell32": synth.cornell32}
AIMED = {"heightfield16": 203, "cornell32": 24}    # the triangle (a) and (b) poison: mid-field; a side of the short box
LEAF_STAND_IN = (100, 101, 102, 103)                # (c) on the host, where no tree is at hand; cornell32: taken modulo its 32 triangles
N_UNIFORM, N_BOXES, N_TRIS, N_AIMED = 8000, 100, 150, 64   # rays per set as in tests/test_gpu_deformable.py; aimed rays per poisoned triangle
SEED_EXPONENT = -18                                 # the seed placeholder's scale, 2^-18: the module docstring says why not 2^-20
DRIFT_OFFSETS = ((5003.7, 4999.3, 5001.9), (50012.0, 49991.0, 50003.0), (8187.0, 8186.0, 8188.5), (2.0 ** 20, 2.0 ** 20, 2.0 ** 20))


def finite_mask(verts):
    return np.isfinite(np.asarray(verts, F32).reshape(len(verts), 9)).all(1)


def strip_nonfinite(verts):
    """(the finite triangles, their original indices)"""
    keep = np.flatnonzero(finite_mask(verts))
    return np.ascontiguousarray(np.asarray(verts, F32)[keep]), keep


def with_verts(sd, verts):
    """`sd` over other vertices: same topology, same attributes"""
    return synth.SceneData(np.ascontiguousarray(verts, F32), sd.normals, sd.tri_material, sd.tri_mesh_id, sd.materials, sd.name, dict(sd.meta),
                           sd.uvs, sd.tangents, sd.material_textures, sd.textures)


def centre(verts):
    p = np.asarray(verts, np.float64).reshape(-1, 3)
    return 0.5 * (p.min(0) + p.max(0))


def scaled(verts, s, axes=(0, 1, 2)):
    """about the box centre on `axes`, in double, rounded once; s = 0 gives exactly zero extent"""
    c, v = centre(verts), np.asarray(verts, np.float64).copy()
    for a in axes:
        v[..., a] = c[a] + (v[..., a] - c[a]) * s
    return v.astype(F32)


def _kind(verts):
    v, _ = strip_nonfinite(verts)
    if len(v) == 0:
        return "nothing"
    area = np.linalg.norm(np.cross(v[:, 1].astype(np.float64) - v[:, 0], v[:, 2].astype(np.float64) - v[:, 0]), axis=1)
    return "finite" if (area > 0).any() else "nothing"


def _step(label, verts, poisoned=()):
    verts = np.ascontiguousarray(verts, F32)
    kind = _kind(verts)
    return Step(label, verts, "poisoned" if len(poisoned) and kind == "finite" else kind, tuple(int(p) for p in poisoned))


def grow(base, placeholder):
    first = np.broadcast_to(base[0, 0], base.shape) if placeholder == "point" else scaled(base, 2.0 ** SEED_EXPONENT)
    steps = [_step(f"placeholder ({placeholder})", first), _step("base", base)]
    steps += [_step(f"x 2^{k}", scaled(base, 2.0 ** k)) for k in (4, 8, 12, 30)]
    return steps + [_step("back to the base", base)]


def shrink(base):
    return [_step("base", base), _step("x 2^-12", scaled(base, 2.0 ** -12)), _step("x 2^-30", scaled(base, 2.0 ** -30)),
            _step("plane", scaled(base, 0.0, (1,))), _step("line", scaled(base, 0.0, (1, 2))), _step("point", scaled(base, 0.0)),
            _step("back to the base", base)]


def drift(base):
    steps = [_step("base", base)]
    for axes, name in (((0,), "x"), ((0, 1, 2), "xyz")):
        for off in DRIFT_OFFSETS:
            o = np.zeros(3, F32)
            o[list(axes)] = np.asarray(off, F32)[list(axes)]
            steps.append(_step(f"drift {name} {off[0]:g}", base + o))
    return steps + [_step("back to the base", base)]


NONFINITE_VALUES = (("-inf", -np.inf), ("+inf", np.inf), ("NaN", np.nan))


def nonfinite(base, aimed, leaf=LEAF_STAND_IN, seed=5):
    """`aimed`: the triangle of (a) and (b); `leaf`: the triangles of (c)"""
    n = len(base)
    rng = np.random.RandomState(seed)
    steps = [_step("base", base)]

    def add(label, verts, poisoned):
        steps.append(_step(label, verts, poisoned))
        steps.append(_step("back to the base", base))
    for name, value in NONFINITE_VALUES:
        for axis in range(3):
            v = base.copy()
            v[aimed, (axis + 1) % 3, axis] = value      # another vertex of the triangle on every axis
            add(f"(a) {name} on {'xyz'[axis]}", v, [aimed])
    v = base.copy()
    v[aimed] = np.nan
    add("(b) a triangle NaN", v, [aimed])
    leaf = sorted({int(t) % n for t in leaf})
    v = base.copy()
    for i, t in enumerate(leaf):
        v[t, i % 3, (i // 3) % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    add("(c) a leaf non-finite", v, leaf)
    picked = np.sort(rng.permutation(n)[:max(1, int(round(0.3 * n)))])
    v = base.copy()
    v[picked, rng.randint(0, 3, len(picked)), rng.randint(0, 3, len(picked))] = np.asarray([np.inf, -np.inf, np.nan], F32)[rng.randint(0, 3, len(picked))]
    add("(d) 30 % non-finite", v, picked)
    v = base.copy()
    v[np.arange(n), rng.randint(0, 3, n), rng.randint(0, 3, n)] = np.asarray([np.inf, -np.inf, np.nan], F32)[rng.randint(0, 3, n)]
    add("(e) every triangle non-finite", v, np.arange(n))
    return steps


def stream(name, family, leaf=LEAF_STAND_IN, base=None):
    base = np.ascontiguousarray(BASES[name]().verts if base is None else base, F32)
    if family == "grow_point":
        return grow(base, "point")
    if family == "grow_seed":
        return grow(base, "seed")
    if family == "shrink":
        return shrink(base)
    if family == "drift":
        return drift(base)
    assert family == "nonfinite", family
    return nonfinite(base, AIMED.get(name, len(base) // 2), leaf)


def shared_scene():
    """two meshes, three instances: the flagged heightfield(16) twice (one turned and stretched), a static box once"""
    field = synth.heightfield(16)
    box = synth.instanced_cornell(1).meshes[1]
    mats = field.materials
    meshes = [synth.SceneData(m.verts, m.normals, m.tri_material * 0, m.tri_mesh_id, mats, m.name) for m in (field, box)]
    inst = [(synth.model_matrix((0.0, 0.0, 0.0)), 0, 1),
            (synth.model_matrix((130.0, 20.0, 10.0), (0.2, 1.0, 0.1), 0.7, (0.5, 1.5, 0.75)), 0, 2),
            (synth.model_matrix((-60.0, 10.0, 40.0), (1.0, 0.3, 0.2), 1.1, (20.0, 30.0, 25.0)), 1, 3)]
    return synth.InstancedSceneData(meshes=meshes, instances=inst, materials=mats, name="shared_edges")


SHARED_FLAGS = [1, 0]


def shared_with(isd, verts):
    """`isd` with the flagged mesh over other vertices"""
    return synth.InstancedSceneData(meshes=[with_verts(isd.meshes[0], verts), isd.meshes[1]], instances=list(isd.instances), materials=isd.materials, name=isd.name)


def step_of(label, verts, poisoned=()):
    return _step(label, verts, poisoned)


# ---------------------------------------------------------------------------------------------------------------- ray sets
def uniform_rays(verts, n, seed):
    """uniform origins in the box of `verts` grown by 5 %, uniform directions, a quarter of them short (1 to 40 % of the diagonal), the rest endless"""
    rng = np.random.RandomState(seed)
    lo, hi, diag = rc.scene_box(verts)
    ext = np.maximum(hi - lo, 1e-3 * diag)
    o = (lo - 0.05 * ext) + rng.uniform(0, 1, (n, 3)) * (1.1 * ext)
    t = np.full(n, np.inf)
    t[:n // 4] = diag * rng.uniform(0.01, 0.4, n // 4)
    return rc.pack(o.astype(F32), rc.unit(rng.normal(size=(n, 3))), t.astype(F32), F32(1e-4 * diag))


def aimed_rays(base, verts, poisoned, seed, per_tri=N_AIMED, max_tris=4):
    """from uniform origins in the box of the finite triangles towards the PRE-poison centroids of up to max_tris poisoned triangles: what tells
    "the triangle is gone" from "its neighbourhood is gone"; returns (rays, the triangle each ray is aimed at)"""
    rng = np.random.RandomState(seed)
    finite, _ = strip_nonfinite(verts)
    lo, hi, diag = rc.scene_box(finite)
    tris = np.asarray(poisoned)[np.sort(rng.permutation(len(poisoned))[:max_tris])]
    tri = np.repeat(tris, per_tri)
    target = np.asarray(base, np.float64)[tri].mean(1)
    o = rng.uniform(lo, hi, (len(tri), 3))
    return rc.pack(o.astype(F32), rc.unit(target - o.astype(F32)), np.full(len(tri), np.inf, F32), 0.0), tri


def ray_sets(step, fresh_boxes, own_boxes=None, seed=0, base=None):
    """The sets of one step, over its FINITE triangles: uniform rays in the current box, grazers of the child boxes (a fresh tree's — api.bvh_child_boxes
    of the finite triangles — and, on the GPU, the refitted scene's own non-empty ones), rays through edges and vertices of the current triangles,
    and for a poisoned step the aimed rays.  A step without finite triangles gets uniform rays in the base's box alone."""
    finite, _ = strip_nonfinite(step.verts)
    if len(finite) == 0:
        return {"uniform": uniform_rays(base, N_UNIFORM, seed)}
    boxes = [sample(fresh_boxes, N_BOXES, seed)]
    if own_boxes is not None:
        ok = np.isfinite(own_boxes["lo"]).all(1) & np.isfinite(own_boxes["hi"]).all(1) & (own_boxes["lo"] <= own_boxes["hi"]).all(1)
        boxes.append(sample(own_boxes[ok], N_BOXES, seed + 1))
    sets = {"uniform": uniform_rays(finite, N_UNIFORM, seed),
            "box_grazers": rc.box_grazers(np.concatenate(boxes), seed=seed + 2),
            "edge_and_vertex": rc.edge_and_vertex_rays(finite, seed=seed + 3, max_tris=N_TRIS)}
    if step.kind == "poisoned":
        sets["aimed"] = aimed_rays(base, step.verts, step.poisoned, seed + 4)[0]
    return sets


def shared_ray_sets(isd, step, fresh_boxes, seed=0):
    """The sets of one step of the flagged mesh inside shared_scene(), in world space (`isd` holds the step's vertices): uniform rays in the box of
    EACH instance of the flagged mesh (under drift the two part ways, and rays across their joint box would meet nothing), uniform rays in the
    static mesh's instance, grazers of a fresh tree's boxes over the flattened scene, rays through edges and vertices of the flattened triangles.
    "static" hits a fair share whatever the step does; the sets together do whenever the step holds something that can be hit."""
    flat = isd.flatten()
    first, _, _, count = isd.layout()
    inst = [flat.verts[f:f + n] for f, n in zip(first, count)]
    sets = {"static": uniform_rays(inst[2], N_UNIFORM // 4, seed + 7)}
    if step.kind != "nothing":
        sets["uniform"] = np.concatenate([uniform_rays(inst[k], N_UNIFORM // 2, seed + k) for k in (0, 1)])
    sets["box_grazers"] = rc.box_grazers(sample(fresh_boxes, N_BOXES, seed), seed=seed + 2)
    sets["edge_and_vertex"] = rc.edge_and_vertex_rays(flat.verts, seed=seed + 3, max_tris=N_TRIS)
    return sets


def point_triangle_distance(p, a, b, c):
    """[n] distances of points p from triangles (a, b, c), all [n][3] float64: the closest point by Voronoi regions (Ericson, Real-Time Collision
    Detection 5.1.5), degenerate triangles included (their regions collapse onto vertices and edges)"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
    bp = p - b
    d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
    cp = p - c
    d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = np.nan_to_num(d1 / (d1 - d3))
        w_ac = np.nan_to_num(d2 / (d2 - d6))
        w_bc = np.nan_to_num((d4 - d3) / ((d4 - d3) + (d5 - d6)))
        den = va + vb + vc
        v_in, w_in = np.nan_to_num(vb / den), np.nan_to_num(vc / den)
    q = a + ab * v_in[:, None] + ac * w_in[:, None]
    sel = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
    q[sel] = (b + (c - b) * w_bc[:, None])[sel]
    sel = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    q[sel] = (a + ac * w_ac[:, None])[sel]
    sel = (d6 >= 0) & (d5 <= d6)
    q[sel] = c[sel]
    sel = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    q[sel] = (a + ab * v_ab[:, None])[sel]
    sel = (d3 >= 0) & (d4 <= d3)
    q[sel] = b[sel]
    sel = (d1 <= 0) & (d2 <= 0)
    q[sel] = a[sel]
    return np.linalg.norm(p - q, axis=1)


def hit_offsets(verts, rays, tuv, prim):
    """How far (float64) the reference's closest hits o + t d lie from the triangles they name, in units of the leaf pad DESIGN.md section 3.3
    promises for these vertices (3e-5 x the diagonal of the finite triangles' box, at least 2^-21 of their largest coordinate).  A hit the fp32
    watertight test grants by rounding alone — a ray IN the plane of a triangle has all three edge functions 0 in exact arithmetic, and
    their rounded signs may agree — lies as far from its triangle as chance has it, beyond any pad."""
    hit = np.flatnonzero(prim >= 0)
    finite, _ = strip_nonfinite(verts)
    step = max(3e-5 * rc.scene_box(finite)[2], 2.0 ** -21 * float(np.abs(finite).max())) if len(finite) else 1.0
    r = rays[hit].astype(np.float64)
    p = r[:, 0:3] + tuv[hit, 0:1].astype(np.float64) * r[:, 4:7]
    t = np.asarray(verts, np.float64)[prim[hit]]
    out = np.zeros(len(rays))
    out[hit] = point_triangle_distance(p, t[:, 0], t[:, 1], t[:, 2]) / float(step)
    return out


def sound(osc, verts, rays):
    """[n] bool: the reference's closest hit of the ray lies within half a leaf pad of the triangle it names (or there is none).  The rest are
    hits by rounding alone (hit_offsets): a triangle far smaller than a float step at the ray's distance — the flagged mesh as a seed seen from
    the static mesh, a 40-unit box seen from 5e9 away after the 2^30 rung, the field 2^20 away — has edge functions that are pure rounding
    noise, and brute force then names triangles hundreds of units from the ray.  No box can be asked to follow those; the shared-scene checks
    leave such rays out and say how many, the flat streams have none (tests/test_deform_cases.py)."""
    tuv, prim = osc.closest_hit(rays, brute_force=True)
    return hit_offsets(verts, rays, tuv, prim) <= 0.5
