"""tests/motion_cases.py, the float64 motion-vector reference of tests/test_gpu_motion_vectors.py, on a case with a closed form (no GPU): a
camera-facing quad translated parallel to the image plane.  With the camera at the origin looking down -z and synth.perspective (y flipped),
a point (x, y, -Z) lands at uv = (0.5 + 0.5 * (f / aspect) * x / Z, 0.5 - 0.5 * f * y / Z); a quad that moved by (tx, ty, 0) since the previous
frame was at (x - tx, y - ty) then, so previous minus current = (-0.5 * (f / aspect) * tx / Z, +0.5 * f * ty / Z) at every texel."""
import math

import numpy as np

import motion_cases as mc
from hybrid_rendering_amd import synth

W, H, Z, FOV, ASPECT = 48, 32, 40.0, 50.0, 1.5
QUAD_ID, OTHER_ID = 7, 3


def _setup(prev_eye=(0.0, 0.0, 0.0)):
    cam = synth.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), fov=FOV, near=1.0, far=1000.0, aspect=ASPECT)
    prev = synth.Camera(tuple(prev_eye), tuple(np.array(prev_eye) + np.array([0.0, 0.0, -1.0])), fov=FOV, near=1.0, far=1000.0, aspect=ASPECT)
    ubo = synth.make_ubo(cam, prev, synth.cornell_light())
    # the depth the synthesiser would write for the plane z = -Z: clip.z / clip.w, one fp32 number per texel
    P = synth.perspective(FOV, ASPECT, 1.0, 1000.0)
    d = np.float32((P[2, 2] * -Z + P[2, 3]) / Z)
    depth = np.full((H, W), d, np.float32)
    depth[:4] = 1.0                                                   # sky rows: no surface
    gb3 = np.zeros((H, W, 4), np.float16)
    gb3[..., 2] = QUAD_ID
    gb3[:, :10, 2] = OTHER_ID                                         # a strip of another instance that stands
    return ubo, depth, gb3


def _translation(t):
    A = np.eye(4)
    A[:3, 3] = t
    return A


def test_a_quad_translated_parallel_to_the_image_plane():
    ubo, depth, gb3 = _setup()
    tx, ty = 1.75, -0.6
    A_prev, A_cur = _translation((3.0, 1.0, 0.0)), _translation((3.0 + tx, 1.0 + ty, 0.0))
    motion, bound, surface, moved = mc.reference(depth, gb3, ubo, {QUAD_ID: (A_prev, A_cur)})
    f = 1.0 / math.tan(math.radians(FOV) / 2)
    expect = np.array([-0.5 * (f / ASPECT) * tx / Z, 0.5 * f * ty / Z])
    assert not surface[:4].any() and surface[4:].all()
    assert np.array_equal(moved, surface & (gb3[..., 2] == QUAD_ID))
    assert moved.sum() == (H - 4) * (W - 10)
    # the quad: the projected shift, previous minus current (it moved to +x: it WAS further left, so the x component is negative)
    assert motion[moved][:, 0].max() < 0.0 and motion[moved][:, 1].max() < 0.0
    err = np.abs(motion[moved] - expect)
    assert (err <= bound[moved]).all(), err.max()
    assert bound[moved].max() < 4e-6 and bound[moved].min() >= mc.FLOOR, "the bound is the depth's ulp and a floor, not slack"
    # the strip that stands, under a camera that stands: exactly 0, and off the surface 0 by definition
    assert np.array_equal(motion[surface & ~moved], np.zeros_like(motion[surface & ~moved]))
    assert np.array_equal(motion[~surface], np.zeros_like(motion[~surface])) and np.array_equal(bound[~surface], np.zeros_like(bound[~surface]))
    # the sign convention is not symmetric: the opposite one is outside the bound everywhere
    assert (np.abs(-motion[moved] - expect) > bound[moved]).any(axis=1).all()


def test_zero_motion_is_exactly_zero():
    ubo, depth, gb3 = _setup()
    A = synth.model_matrix((5.0, -2.0, 1.0), (0.3, 1.0, -0.2), 0.7, (1.5, 0.8, 2.0))
    A = mc.mat4(A)
    motion, bound, surface, moved = mc.reference(depth, gb3, ubo, {QUAD_ID: (A, A.copy())})
    assert not moved.any()
    assert np.array_equal(motion, np.zeros_like(motion))
    assert np.array_equal(bound[surface], np.full_like(bound[surface], mc.FLOOR))


def test_camera_motion_alone_and_the_default_pair():
    """a camera that moved by +c sees a standing world move by -c: the same closed form through prev_view_proj; `default` moves every id"""
    c = (0.9, 0.4, 0.0)
    ubo, depth, gb3 = _setup(prev_eye=c)          # the previous camera sat at +c: the world WAS at -c relative to it
    motion, bound, surface, moved = mc.reference(depth, gb3, ubo, {})
    f = 1.0 / math.tan(math.radians(FOV) / 2)
    expect = np.array([-0.5 * (f / ASPECT) * c[0] / Z, 0.5 * f * c[1] / Z])
    assert not moved.any()
    assert (np.abs(motion[surface] - expect) <= bound[surface]).all()
    # an object that moved WITH the camera stands still on screen
    motion2, bound2, _, moved2 = mc.reference(depth, gb3, ubo, {}, default=(_translation((0.0, 0.0, 0.0)), _translation((-c[0], -c[1], 0.0))))
    assert np.array_equal(moved2, surface)
    assert (np.abs(motion2[surface]) <= bound2[surface]).all()
