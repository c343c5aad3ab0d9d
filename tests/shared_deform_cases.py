"""The scenes, deformation steps and ray sets of tests/test_instances_shared_deform_host.py (CPU: the oracle alone checks that they can tell a
right answer from a wrong one) and tests/test_gpu_instances_shared_deform.py (the same sets against hr_scene_update_meshes).

The scene: synth.instanced_cornell(4) plus two deforming meshes — FIELD, a 24 x 24 heightfield (1152 triangles: its tree has a level of 64 nodes, wider than the 32 the one-workgroup
launch keeps, which takes the per-level refit launch) placed four times, and BOX, a 12-triangle cube (refitted by the one-workgroup launch
alone) placed three times."""
import numpy as np

from hybrid_rendering_amd import synth

SEED = 6
FIELD, BOX = 3, 4                       # mesh indices of the two deforming meshes
FLAGS = [0, 0, 0, 1, 1]
N_RAYS = 20000
STEPS = [(kind, frame) for kind in ("wave", "twist", "collapse") for frame in (1, 2, 3)]


def scene(seed=SEED):
    base = synth.instanced_cornell(4, seed=seed)
    field = synth.heightfield(24, size=30.0, height=4.0)
    assert field.n_tris == 1152
    box = synth.instanced_cornell(1).meshes[1]
    assert box.n_tris == 12
    rng = np.random.RandomState(seed)
    inst = list(base.instances)
    for i in range(4):
        at = (float(rng.uniform(10, 60)), 12.0 + 18.0 * i, float(rng.uniform(10, 60)))
        inst.append((synth.model_matrix(at, (0.0, 1.0, 0.0), float(rng.uniform(0, 6.28)), (1.0, 1.0 + 0.5 * i, 0.8)), FIELD, 20 + i))
    for i in range(3):
        at = tuple(float(x) for x in rng.uniform(20, 80, 3))
        inst.append((synth.model_matrix(at, tuple(rng.uniform(-1, 1, 3)), float(rng.uniform(0, 6.28)), tuple(float(x) for x in rng.uniform(6, 14, 3))), BOX, 30 + i))
    meshes = list(base.meshes) + [field, box]
    meshes = [synth.SceneData(m.verts, m.normals, m.tri_material * 0 if k >= 3 else m.tri_material, m.tri_mesh_id, base.materials, m.name) for k, m in enumerate(meshes)]
    return synth.InstancedSceneData(meshes=meshes, instances=inst, materials=base.materials, name="shared_deform")


def moved(isd, step):
    """matrices of update `step`: every second instance of the deforming meshes drifts and turns (hr_scene_update_instances between mesh updates)"""
    mats = isd.matrices().copy()
    for i, (_, k, _) in enumerate(isd.instances):
        if k >= FIELD and i % 2 == 0:
            mats[i, 12:15] += np.float32(1.5 * step) * np.array([1.0, -0.4, 0.7], np.float32)
    return mats


def instance_boxes(isd, mats=None):
    """[n_instances][2][3]: world bounds of every instance's vertices under flatten()"""
    flat = isd.flatten(mats)
    first, _, _, n = isd.layout()
    out = np.zeros((len(first), 2, 3), np.float32)
    for i, (f, k) in enumerate(zip(first, n)):
        if k:
            v = flat.verts[f:f + k].reshape(-1, 3)
            out[i] = v.min(0), v.max(0)
    return out


def rays(isd, mats, n=N_RAYS, seed=1):
    """a third uniform in the room (a quarter of those short), a third from the room towards points on the deforming instances' CURRENT surfaces,
    a third short segments around those points that mostly miss: hit fraction in the middle of [0.10, 0.90]"""
    rng = np.random.RandomState(seed)
    flat = isd.flatten(mats)
    first, _, _, cnt = isd.layout()
    deforming = np.concatenate([np.arange(f, f + k) for (f, k), (_, m, _) in zip(zip(first, cnt), isd.instances) if m >= FIELD])
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(5.0, 95.0, (n, 3))
    d = rng.normal(size=(n, 3))
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 3], r[:, 7] = 1e4, 0.01
    a, b = n // 3, 2 * (n // 3)
    r[:a // 4, 3] = rng.uniform(3, 40, a // 4)
    tri = flat.verts[deforming[rng.randint(0, len(deforming), n - a)]].astype(np.float64)
    w = rng.dirichlet((1.0, 1.0, 1.0), n - a)
    target = (tri * w[:, :, None]).sum(1)
    to = target - r[a:, :3]
    dist = np.linalg.norm(to, axis=1, keepdims=True)
    r[a:, 4:7] = to / np.maximum(dist, 1e-9)
    # the last third: segments that start 0.5 to 4 units before the surface point and end within +- 1 unit of it
    near = rng.uniform(0.5, 4.0, (n - b, 1))
    r[b:, :3] = target[b - a:] - r[b:, 4:7] * near
    r[b:, 3] = (near[:, 0] + rng.uniform(-1.0, 1.0, n - b)).astype(np.float32)
    return r


def stale_boxes(isd, mats):
    """[n_instances][2][3]: what an instance's world box would be had a mesh update NOT reached the host — the eight corners of the UNDEFORMED
    mesh's object-space bounds through the instance's current matrix (the construction of csrc/instances.hip instance_boxes)"""
    out = np.zeros((len(isd.instances), 2, 3), np.float64)
    for i, ((_, k, _), m) in enumerate(zip(isd.instances, np.asarray(mats, np.float64).reshape(-1, 16))):
        if isd.meshes[k].n_tris == 0:
            continue
        lo, hi = [b.astype(np.float64) for b in isd.meshes[k].bounds()]
        c = np.array([[(lo, hi)[(j >> a) & 1][a] for a in range(3)] for j in range(8)])
        M = m.reshape(4, 4).T
        w = c @ M[:3, :3].T + M[:3, 3]
        out[i] = w.min(0), w.max(0)
    return out


def step_inputs(isd, step):
    """(deformed InstancedSceneData, matrices, rays) of STEPS[step]"""
    kind, frame = STEPS[step]
    d = synth.deform_meshes(isd, frame, kind, (FIELD, BOX))
    mats = moved(isd, step)
    return d, mats, rays(d, mats, seed=step + 1)
