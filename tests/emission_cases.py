"""Inputs of the emissive-material tests (tests/test_emission_cases.py validates them without a GPU; tests/test_gpu_emission.py runs them).

One small world — a closed Cornell-like box, two cubes, a one-triangle emitter and a textured emissive quad and a dark panel under the ceiling, 125 triangles — as a
synth.InstancedSceneData, so that the same world-space triangles exist as a flat scene (its flatten()), a private-copy instanced scene and a
shared instanced scene.  Materials: 0 white, 1 red, 2 green (the room), 3 grey (the cubes), 4 the one-triangle emitter, 5 the quad, 6 the ceiling panel (dark unless a test lights it).
Mesh ids: 1 the room, 2 and 3 the cubes, 4 the emitter, 5 the quad, 6 the panel: every mesh id but the room's has one material."""
import dataclasses

import numpy as np

from hybrid_rendering_amd import synth

import emission_reference as er

F = np.float32
S = 10.0                                  # the room is [0, S]^3
N_MATERIALS, EMITTER, QUAD, CUBES, PANEL = 7, 4, 5, 3, 6
N_RAYS, RAY_SEED = 4096, 23
TEX_EMISSIVE, TEX_ALBEDO_QUAD, TEX_HOLE = 0, 1, 2   # the scene's textures
MESH_IDS = (1, 2, 3, 4, 5, 6)


def _grid(p0, du, dv, n):
    """an n x n grid of quads over the parallelogram p0, du, dv: (verts [2n^2][3][3], uvs [2n^2][3][2] in [0, 1]^2)"""
    p0, du, dv = (np.asarray(a, np.float64) for a in (p0, du, dv))
    V, U = [], []
    for j in range(n):
        for i in range(n):
            c = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            P = [p0 + du * (a / n) + dv * (b / n) for a, b in c]
            T = [(a / n, b / n) for a, b in c]
            for k in ((0, 1, 2), (0, 2, 3)):
                V.append([P[m] for m in k]); U.append([T[m] for m in k])
    return np.asarray(V, F), np.asarray(U, F)


def _mesh(verts, uvs, mats, name):
    verts = np.ascontiguousarray(verts, F)
    fn = np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]).astype(np.float64)
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    return synth.SceneData(verts, np.ascontiguousarray(np.repeat(fn[:, None, :], 3, 1), F), np.asarray(mats, np.uint32), np.zeros(len(verts), np.uint32),
                           materials(), name, {}, uvs=np.ascontiguousarray(uvs, F))


def materials(emissive=True):
    """[7][8]: albedo rgb, metallic, roughness, emissive rgb.  The emitter's constant is in the description; the quad's is replaced by its texture."""
    m = np.array([[0.75, 0.75, 0.75, 0.0, 0.6, 0, 0, 0], [0.7, 0.15, 0.1, 0.0, 0.6, 0, 0, 0], [0.15, 0.6, 0.15, 0.0, 0.6, 0, 0, 0],
                  [0.5, 0.5, 0.55, 0.0, 0.4, 0, 0, 0], [0.2, 0.2, 0.2, 0.0, 0.8, 2.5, 1.75, 0.5], [0.3, 0.3, 0.3, 0.0, 0.8, 0.125, 0.25, 0.375],
                  [0.6, 0.6, 0.6, 0.0, 0.7, 0, 0, 0]], F)
    if not emissive:
        m[:, 5:] = 0
    return m


def textures():
    rng = np.random.RandomState(41)
    emissive = rng.randint(0, 256, (4, 4, 4)).astype(np.uint8)      # 4 x 4: (k + 0.5) / 4 is exact, so bilinear weights of exactly 0 and 1 occur
    emissive[0, 0, :3] = (255, 0, 128); emissive[0, 1, :3] = (0, 255, 7)
    albedo = np.full((2, 2, 4), 255, np.uint8); albedo[..., :3] = (90, 80, 70)
    hole = np.full((2, 2, 4), 0, np.uint8); hole[..., :3] = 200     # alpha 0 everywhere: a material on it under a cutoff does not exist for the ray
    return [np.ascontiguousarray(t) for t in (emissive, albedo, hole)]


def instanced(emissive=True):
    """the world as meshes + instances (6 instances of 5 meshes)"""
    walls = [((0, 0, 0), (S, 0, 0), (0, 0, S), 0), ((0, S, 0), (0, 0, S), (S, 0, 0), 0), ((0, 0, 0), (0, S, 0), (S, 0, 0), 0),      # floor, ceiling, back (z = 0)
             ((0, 0, S), (S, 0, 0), (0, S, 0), 0), ((0, 0, 0), (0, 0, S), (0, S, 0), 1), ((S, 0, 0), (0, S, 0), (0, 0, S), 2)]      # front, left red, right green
    V, U, M = [], [], []
    for p0, du, dv, mat in walls:
        v, u = _grid(p0, du, dv, 2)
        V.append(v); U.append(u); M += [mat] * len(v)
    room = _mesh(np.concatenate(V), np.concatenate(U), M, "room")                                   # 48 triangles
    V, U = [], []
    for p0, du, dv in (((-.5, -.5, -.5), (0, 0, 1), (0, 1, 0)), ((.5, -.5, -.5), (0, 1, 0), (0, 0, 1)), ((-.5, -.5, -.5), (1, 0, 0), (0, 0, 1)),
                       ((-.5, .5, -.5), (0, 0, 1), (1, 0, 0)), ((-.5, -.5, -.5), (0, 1, 0), (1, 0, 0)), ((-.5, -.5, .5), (1, 0, 0), (0, 1, 0))):
        v, u = _grid(p0, du, dv, 1 if len(V) % 2 else 2)
        V.append(v); U.append(u)
    cube = _mesh(np.concatenate(V), np.concatenate(U), [CUBES] * sum(len(v) for v in V), "cube")      # 3 * 8 + 3 * 2 = 30 triangles, instanced twice
    tri = _mesh(np.array([[[-1, 0, -1], [1, 0, -1], [0, 0, 1]]], F), np.array([[[0, 0], [1, 0], [0.5, 1]]], F), [EMITTER], "emitter")
    qv, qu = _grid((-1, -1, 0), (2, 0, 0), (0, 2, 0), 2)
    qu = qu * F(3.0) - F(1.25)                                                                       # [-1.25, 1.75]^2: all four sign quadrants, REPEAT both ways
    qu[0, 0] = (0.125, 0.375)                                                                        # vertex 0 of triangle 0 sits on a texel centre of the 4 x 4 texture
    quad = _mesh(qv, qu, [QUAD] * len(qv), "quad")                                                   # 8 triangles
    pv, pu = _grid((1, 0, 1), (0, 0, 8), (8, 0, 0), 2)
    panel = _mesh(pv, pu, [PANEL] * len(pv), "panel")                                                # 8 triangles, 8 x 8
    inst = [(synth.model_matrix(), 0, 1),
            (synth.model_matrix((3.0, 1.5, 3.5), (0, 1, 0), 0.5, (2.0, 3.0, 2.0)), 1, 2),
            (synth.model_matrix((7.0, 1.0, 6.5), (1, 2, 0.5), 0.9, 2.0), 1, 3),
            (synth.model_matrix((5.0, 9.5, 5.0), (0, 1, 0), 0.3, 1.5), 2, 4),                         # the one-triangle emitter under the ceiling
            (synth.model_matrix((8.5, 5.0, 2.0), (0, 1, 0), -0.9, 1.6), 3, 5),                        # the textured quad, standing near the green wall
            (synth.model_matrix((0.0, S - 0.05, 0.0)), 4, 6)]                                         # the panel, just under the ceiling
    mt = np.full((N_MATERIALS, 6), -1, np.int32)
    mt[:, 4], mt[:, 5] = 1, 2
    mt[QUAD, 0] = TEX_ALBEDO_QUAD
    return synth.InstancedSceneData(meshes=[room, cube, tri, quad, panel], instances=inst, materials=materials(emissive), name="emission_world", material_textures=mt,
                                    textures=textures())


EMISSIVE_TEX = np.array([-1, -1, -1, -1, -1, TEX_EMISSIVE, -1], np.int32)      # the quad's emissive texture; everything else constant
NO_TEX = np.full(N_MATERIALS, -1, np.int32)


def emissive_rgb(isd):
    return np.ascontiguousarray(np.asarray(isd.materials, F)[:, 5:8])


def per_mesh_id_rgb():
    """one constant emitter colour per mesh id: the three room materials share one.  Returns (rgb [7][3], table mesh id -> rgb)"""
    table = {1: (0.25, 0.0, 0.5), 2: (1.5, 0.75, 0.0), 3: (1.5, 0.75, 0.0), 4: (3.0, 2.0, 1.0), 5: (0.0, 0.625, 0.125), 6: (0.0, 0.0, 0.0)}
    rgb = np.array([table[1], table[1], table[1], table[2], table[4], table[5], table[6]], F)
    return rgb, {k: np.array(v, F) for k, v in table.items()}


def rays(n=N_RAYS, seed=RAY_SEED):
    """[n][8] float32 (origin, t_max, direction, t_min): three quarters from inside the room in every direction (every one hits), a quarter from
    outside aimed past it or short (misses)"""
    rng = np.random.RandomState(seed)
    o = rng.uniform(0.3, S - 0.3, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 8
    aim = np.array([[5.0, 9.5, 5.0], [8.5, 5.0, 2.0]])[rng.randint(0, 2, 3 * k)] + rng.uniform(-1.2, 1.2, (3 * k, 3)) * (1, 0.2, 1)   # towards the two emitters
    d[:3 * k] = aim - o[:3 * k]; d[:3 * k] /= np.linalg.norm(d[:3 * k], axis=1, keepdims=True)
    r = np.zeros((n, 8), F)
    r[:, 0:3], r[:, 4:7], r[:, 3] = o, d, 1.0e4
    r[-k:, 3] = 0.05                                   # too short to reach anything: misses
    r[-2 * k:-k, 0:3] += (0, 3 * S, 0)                 # from above the closed room, any direction but down-ish is a miss; the others hit the ceiling's back
    return r


def attribute_index(isd, prim):
    """hr_trace_closest_hit's triangle numbers (instance order, then mesh order; -1: a miss) -> indices into isd.mesh_arrays() (-1: a miss)"""
    first, base, _, n = isd.layout()
    prim = np.asarray(prim, np.int64)
    i = np.clip(np.searchsorted(first.astype(np.int64), prim, side="right") - 1, 0, len(first) - 1)
    return np.where(prim >= 0, base.astype(np.int64)[i] + (prim - first.astype(np.int64)[i]), -1)


def expected(isd, rgb, tex, scale, prim, tuv):
    """emission_reference.emission for hits in hr_trace_closest_hit's conventions on any kind of scene made from `isd`"""
    ma = isd.mesh_arrays()
    return er.emission(ma["material"], ma["uvs"], isd.textures, rgb, tex, scale, attribute_index(isd, prim), tuv[:, 1], tuv[:, 2])


def crafted_hits(isd):
    """hits no ray needs to find: the quad's vertex that sits on a texel centre (bilinear weights exactly 1 and 0), its neighbours, a vertex of every
    quad triangle.  (prim int32 [k], tuv float32 [k][3])"""
    first, _, _, n = isd.layout()
    q0 = int(first[4])
    prim = [q0, q0, q0] + [q0 + t for t in range(int(n[4]))] + [int(first[3]), -1]
    uv = [(0, 0), (1, 0), (0.25, 0.5)] + [(0, 1)] * int(n[4]) + [(0.25, 0.25), (0.5, 0.25)]
    tuv = np.zeros((len(prim), 3), F)
    tuv[:, 0], tuv[:, 1:] = 1.0, np.asarray(uv, F)
    return np.asarray(prim, np.int32), tuv


def with_hidden_material(isd, material):
    """a copy whose `material` has the all-transparent texture as its albedo: under a cutoff above 0 its triangles do not exist for the ray class"""
    mt = np.array(isd.material_textures, np.int32).copy()
    mt[material, 0] = TEX_HOLE
    return dataclasses.replace(isd, material_textures=mt)


def without_material(isd, material):
    """the world created without the triangles of `material` (meshes that hold nothing else keep zero triangles' worth: they are dropped with their instances)"""
    meshes, keep = [], {}
    for k, m in enumerate(isd.meshes):
        sel = np.asarray(m.tri_material) != material
        if sel.any():
            keep[k] = len(meshes)
            meshes.append(dataclasses.replace(m, verts=m.verts[sel], normals=m.normals[sel], tri_material=m.tri_material[sel], tri_mesh_id=m.tri_mesh_id[sel], uvs=m.uvs[sel]))
    inst = [(mat, keep[k], mid) for mat, k, mid in isd.instances if k in keep]
    return dataclasses.replace(isd, meshes=meshes, instances=inst)


def cutoffs_for(material):
    c = np.zeros(N_MATERIALS, F)
    c[material] = 0.5
    return c


def camera(aspect):
    """from inside the room near the front wall, looking at the back and up: the emitter, the panel, the quad, both cubes, the floor and three walls are in view"""
    return synth.Camera((5.0, 5.0, 9.6), (5.2, 6.5, 0.0), fov=90.0, aspect=aspect, near=0.05, far=60.0)


def camera_outside(aspect):
    """from outside the closed room: its front wall in the middle of the image, sky around it"""
    return synth.Camera((6.0, 7.0, 34.0), (5.0, 5.0, 5.0), fov=50.0, aspect=aspect, near=0.5, far=200.0)


def black(isd):
    """every albedo 0, metallic 0 (item 4: with light intensity 0 and a black sky only E is left)"""
    m = np.asarray(isd.materials, F).copy()
    m[:, :4] = 0
    mt = np.array(isd.material_textures, np.int32).copy()
    mt[:, :4] = -1                                      # no albedo texture either; the textures stay, for the emissive one
    return dataclasses.replace(isd, materials=m, material_textures=mt)


# ---- the passes' set-up, shared by the CPU check of the clamp condition and the GPU tests -----------------------------------------------------------
REFL_W, REFL_H = 64, 40
PROBES, RAYS_PER_PROBE = (3, 3, 3), 32
# The additivity test needs texels under the reflections' 0.7 clamp: the point light's intensity is chosen so that the ORACLE's trace image of the
# emission-free world has at most 10 % of its traced texels at the clamp (asserted by tests/test_emission_cases.py, on the CPU)
LIT_INTENSITY = 20.0
LIGHT_POSITION = (4.0, 7.5, 6.0)


def light(intensity=LIT_INTENSITY):
    """a point light inside the closed room (a directional light cannot reach into it)"""
    return synth.make_light(synth.LIGHT_POINT, position=LIGHT_POSITION, radius=0.05, intensity=intensity)


def ddgi_grid(probes=PROBES, rays=RAYS_PER_PROBE):
    """probes at 1.5, 5 and 8.5 along every axis: all 27 inside the room"""
    from hybrid_rendering_amd import synth_env
    return synth_env.ddgi_uniforms((1.5, 1.5, 1.5), (5.0, 5.0, 5.0), probe_counts=probes, rays_per_probe=rays, normal_bias=1.0)


def all_mirrors(cur):
    """gb3.x = 0.03 on every surface pixel: each traces a mirror reflection ray"""
    cur["gb3"][..., 0][cur["depth"] != 1.0] = np.float16(0.03).view(np.uint16)
    return cur


def panel_rgb(value=4.0):
    """item 6: only the ceiling panel emits"""
    rgb = np.zeros((N_MATERIALS, 3), F)
    rgb[PANEL] = value
    return rgb
