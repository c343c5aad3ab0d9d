"""A float64 reference for the motion vectors of hr_gbuffer_raycast_motion under RIGID or AFFINE motion, which needs no ray tracing (no GPU, no
oracle): tests/test_motion_cases.py pins it on a closed form, tests/test_gpu_motion_vectors.py holds the synthesiser against it.

For a surface texel the world position P comes back from the GPU's own `depth` through the inverse view-projection; the GB3 mesh id names the
instance, whose previous and current object -> world maps A_prev, A_cur are known to the test; prev_P = A_prev * A_cur^-1 * P; the motion is
uv(prev_view_proj * prev_P) - uv(view_proj * P), uv = ndc * 0.5 + 0.5 — "previous minus current", the convention of the G-buffer kernels
(csrc/api.hip: pack_h2(px - cx, py - cy)).

The bound that comes with it is the reference's OWN uncertainty: `depth` is an fp32 number, known to an ulp or so, and everything else here is
float64.  Per texel and component: twice the spread of the result over depth - 1 ulp, depth, depth + 1 ulp, plus 2^-20 (a dozen roundings of the
fp32 uv arithmetic at values below 2; one ulp at 1 is 2^-23)."""
import numpy as np

FLOOR = 2.0 ** -20


def mat4(m16) -> np.ndarray:
    """column-major 16 floats (hr_ubo, hr_instance.model_matrix) -> float64 [4][4], M @ column vector"""
    return np.asarray(m16, np.float64).reshape(4, 4).T.copy()


def _uv(M, P):
    c = P @ M.T
    return c[..., :2] / c[..., 3:4] * 0.5 + 0.5


def _motion_at(depth64, VP_inv, VP, PVP, T):
    h, w = depth64.shape
    x, y = (np.arange(w, dtype=np.float64) + 0.5) / w, (np.arange(h, dtype=np.float64) + 0.5) / h
    ndc = np.stack([np.broadcast_to(2.0 * x[None, :] - 1.0, (h, w)), np.broadcast_to(2.0 * y[:, None] - 1.0, (h, w)), depth64, np.ones((h, w))], -1)
    P = ndc @ VP_inv.T
    P = P / P[..., 3:4]
    prev_P = np.einsum("hwij,hwj->hwi", T, P) if T.ndim == 4 else P @ T.T
    return _uv(PVP, prev_P) - _uv(VP, P)


def reference(depth, gb3, ubo, transforms, default=None):
    """depth: float32 [h][w] as the synthesiser wrote it; gb3: [h][w][4] float16 (or its uint16 bits), .z = mesh id; ubo: synth.UBO_DTYPE record;
    transforms: {mesh id: (A_prev, A_cur)}, float64 [4][4] each (mat4()); default: the pair of every other id (None: it did not move).
    Returns (motion [h][w][2] float64, bound [h][w][2] float64, surface [h][w] bool, moved [h][w] bool); motion / bound are 0 off the surface."""
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    ids = np.asarray(gb3)
    ids = (ids.view(np.float16) if ids.dtype == np.uint16 else ids)[..., 2].astype(np.float64)
    surface = depth < np.float32(1.0)
    VP, PVP = mat4(ubo["view_proj"]), mat4(ubo["prev_view_proj"])
    VP_inv = np.linalg.inv(VP)
    eye = np.eye(4)
    T = np.broadcast_to(eye, (h, w, 4, 4)).copy()
    moved = np.zeros((h, w), bool)
    pairs = dict(transforms)
    for i in np.unique(ids[surface]):
        pair = pairs.get(int(i), default)
        if pair is None:
            continue
        A_prev, A_cur = (np.asarray(a, np.float64) for a in pair)
        if np.array_equal(A_prev, A_cur):
            continue                                  # it stands: the identity EXACTLY, not A * A^-1
        sel = surface & (ids == i)
        T[sel] = A_prev @ np.linalg.inv(A_cur)
        moved |= sel
    one = np.float32(1.0)
    d0 = depth.astype(np.float64)
    dm, dp = np.nextafter(depth, -one).astype(np.float64), np.nextafter(depth, one + one).astype(np.float64)
    r = np.stack([_motion_at(d, VP_inv, VP, PVP, T) for d in (dm, d0, dp)])
    motion = r[1]
    bound = 2.0 * (r.max(0) - r.min(0)) + FLOOR
    motion[~surface] = 0.0
    bound[~surface] = 0.0
    return motion, bound, surface, moved
