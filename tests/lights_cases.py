"""Inputs of the extra-lights tests (tests/test_gpu_lights.py runs them; tests/test_lights_host.py checks the world without a GPU).

The world is tests/emission_cases.py's room at its scale — [0, 10]^3, two cubes and the textured quad, as a synth.InstancedSceneData, so that the
same world-space triangles exist as a flat, a private-copy and a shared scene — with two changes that make LIGHTS reach its surfaces: the room's
walls are wound INWARDS (emission_cases winds them outwards: N . Wi is 0 for every light inside), and the ceiling, its panel and the one-triangle
emitter are left out, so that a directional light shines in from above.  `partitioned()` puts the ceiling back and a thick wall across the
middle of the room (the cube mesh, scaled), for the test in which a lamp lights one half."""
import dataclasses

import numpy as np

from hybrid_rendering_amd import synth

import emission_cases as ec

F = np.float32
S = ec.S
N_MATERIALS, CUBES = ec.N_MATERIALS, ec.CUBES
W, H = ec.REFL_W, ec.REFL_H                       # 64 x 40
RAGGED = (61, 37)
PROBES, RAYS_PER_PROBE = ec.PROBES, ec.RAYS_PER_PROBE
HR_MAX_LIGHTS = 256


def _inwards(mesh, keep=None):
    """the mesh with every triangle's winding and normals turned round (and only the triangles `keep` selects)"""
    sel = np.ones(len(mesh.verts), bool) if keep is None else keep
    o = [0, 2, 1]
    return dataclasses.replace(mesh, verts=np.ascontiguousarray(mesh.verts[sel][:, o]), normals=np.ascontiguousarray(-mesh.normals[sel][:, o]),
                               tri_material=mesh.tri_material[sel], tri_mesh_id=mesh.tri_mesh_id[sel], uvs=np.ascontiguousarray(mesh.uvs[sel][:, o]))


def world(ceiling=False):
    """room (inward walls; 40 triangles without the ceiling, 48 with), two cubes, the quad"""
    base = ec.instanced(emissive=False)
    room, cube, _, quad, _ = base.meshes
    keep = np.ones(len(room.verts), bool)
    if not ceiling:
        keep[8:16] = False                        # emission_cases builds the ceiling second, 8 triangles
    inst = [base.instances[0], base.instances[1], base.instances[2], (base.instances[4][0], 2, 5)]
    return dataclasses.replace(base, meshes=[_inwards(room, keep), cube, quad], instances=inst, name="lights_world")


def partitioned():
    """the closed room with a wall 0.5 thick across x = 5 that pokes through floor, ceiling, front and back: no path from one half to the other"""
    w = world(ceiling=True)
    inst = [w.instances[0], (synth.model_matrix((5.0, 5.0, 5.0), (0, 1, 0), 0.0, (0.5, S + 0.4, S + 0.4)), 1, 2)]
    return dataclasses.replace(w, meshes=w.meshes[:2], instances=inst, name="lights_partitioned")


def hidden_cubes(isd):
    """the cutout variant: the cubes' albedo is the all-transparent texture; under `cutoffs()` they do not exist for any ray class"""
    return ec.with_hidden_material(isd, CUBES)


def cutoffs():
    return ec.cutoffs_for(CUBES)


def camera(aspect):
    return ec.camera(aspect)


def camera_outside(aspect):
    """sky around the room"""
    return ec.camera_outside(aspect)


# ---- the lights ---------------------------------------------------------------------------------------------------------------------------------
def directional(intensity=3.0, to_light=(0.3, 0.9, 0.2), colour=(1.0, 0.9, 0.8)):
    return synth.make_light(synth.LIGHT_DIRECTIONAL, direction_to_light=to_light, radius=0.02, color=colour, intensity=intensity)


def point(intensity=20.0, position=ec.LIGHT_POSITION, colour=(1.0, 1.0, 1.0)):
    return synth.make_light(synth.LIGHT_POINT, position=position, radius=0.05, color=colour, intensity=intensity)


def spot(intensity=40.0, position=(5.0, 8.0, 5.5), to_light=(0.1, 1.0, 0.05), colour=(0.8, 1.0, 0.9), inner=35.0, outer=60.0):
    return synth.make_light(synth.LIGHT_SPOT, direction_to_light=to_light, position=position, radius=0.05, color=colour, intensity=intensity, cone_inner_deg=inner, cone_outer_deg=outer)


LIGHTS = dict(directional=directional, point=point, spot=spot)


def dark(light):
    """the same light at intensity 0: the UBO light of the swapped scene"""
    d = np.array(light, F).copy()
    d[3] = 0.0
    return d


def records(*lights):
    """hr_light records [n, 4, 4] of flat 16-float lights"""
    return np.stack([np.asarray(l, F).reshape(4, 4) for l in lights]) if lights else np.zeros((0, 4, 4), F)


def padded(lit, n, seed=11):
    """a list of n records that holds the lights `lit` at seeded places, in their order, and lights of intensity 0 (of every type, anywhere in and
    around the room) everywhere else.  Returns (records [n, 4, 4], the places)"""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, 4, 4), F)
    for k in range(n):
        kind = (synth.LIGHT_DIRECTIONAL, synth.LIGHT_POINT, synth.LIGHT_SPOT)[k % 3]
        out[k] = synth.make_light(kind, direction_to_light=rng.normal(size=3), position=rng.uniform(-2, S + 2, 3), radius=0.05, color=rng.uniform(0, 1, 3), intensity=0.0).reshape(4, 4)
    at = np.sort(rng.choice(n, len(lit), replace=False))
    for k, l in zip(at, lit):
        out[k] = np.asarray(l, F).reshape(4, 4)
    return out, at


def disjoint_spots():
    """two narrow spots shining at the back wall (z = 0, what the camera looks at) from z = 4, at x = 2.5 and x = 7.5, y = 6: a cone of 25 degrees is
    4 tan 25 = 1.87 wide at the wall, so one lights only x in (0.6, 4.4) and the other only x in (5.6, 9.4), between y = 4.1 and 7.9; outside its
    cone a spot's smoothstep is exactly 0.  No point is inside both."""
    a = spot(60.0, position=(2.5, 6.0, 4.0), to_light=(0.0, 0.0, 1.0), inner=15.0, outer=25.0, colour=(1.0, 0.5, 0.25))
    b = spot(60.0, position=(7.5, 6.0, 4.0), to_light=(0.0, 0.0, 1.0), inner=15.0, outer=25.0, colour=(0.25, 0.5, 1.0))
    return a, b


def overlapping():
    """three lights that share most of the room"""
    return directional(1.5), point(15.0), spot(30.0)
