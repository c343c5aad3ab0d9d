"""include/hr_skin.h's contract in numpy float32, one rounding per operation (every intermediate is a float32 array, numpy fuses nothing), sums
in the order written — the restatement csrc/skin_math.h is held to, bit for bit, on the host (tests/test_skin_cases.py) and on the GPU
(tests/test_gpu_skin.py).  Also the containment check of hr_skin_bounds."""
import numpy as np

F = np.float32


def rows_of(matrices):
    """[n_joints][16] column-major -> J[j][r][c] for r = 0..2 (the last row is not read)"""
    m = np.asarray(matrices, F).reshape(-1, 4, 4)      # m[j][c][r]
    return np.ascontiguousarray(m.transpose(0, 2, 1)[:, :3, :])


def morph(v, deltas, morph_weights):
    """v = v + mw[t] * d[t] for t in order (the product rounded, then the sum); mw[t] == 0 is skipped"""
    v = np.asarray(v, F).reshape(-1, 3).copy()
    if deltas is None or morph_weights is None:
        return v
    d = np.asarray(deltas, F).reshape(len(deltas), -1, 3)
    for t, mw in enumerate(np.asarray(morph_weights, F).reshape(-1)):
        if mw == 0:
            continue
        prod = (mw * d[t]).astype(F)
        v = (v + prod).astype(F)
    return v


def blend(joints, weights, matrices):
    """M[i][r][c] over the slots whose weight is not zero, in slot order; a skipped slot's joint is not looked up"""
    J = rows_of(matrices)
    j = np.asarray(joints).reshape(-1, 4).astype(np.int64)
    w = np.asarray(weights, F).reshape(-1, 4)
    M = np.zeros((len(w), 3, 4), F)
    first = np.ones(len(w), bool)
    for k in range(4):
        live = w[:, k] != 0
        idx = np.where(live, j[:, k], 0)
        idx = np.where(idx < len(J), idx, 0)     # only a skipped slot can be out of range (hr_skin_check_desc)
        with np.errstate(all="ignore"):
            T = (w[:, k, None, None] * J[idx]).astype(F)
            S = (M + T).astype(F)
        M = np.where(live[:, None, None], np.where(first[:, None, None], T, S), M).astype(F)
        first &= ~live
    return M


def pose(arrays, matrices, morph_weights=None):
    """(positions, normals), [n_tris,3,3] float32 each.  arrays: dict with verts, normals, joints, weights and optionally target_positions /
    target_normals ([n_targets,n_tris,3,3])"""
    verts = np.asarray(arrays["verts"], F)
    tp, tn = arrays.get("target_positions"), arrays.get("target_normals")
    p = morph(verts, tp, morph_weights)
    n = morph(arrays["normals"], tn if tp is not None else None, morph_weights)
    M = blend(arrays["joints"], arrays["weights"], matrices)
    with np.errstate(all="ignore"):
        op = np.stack([((((M[:, r, 0] * p[:, 0]).astype(F) + (M[:, r, 1] * p[:, 1]).astype(F)).astype(F) + (M[:, r, 2] * p[:, 2]).astype(F)).astype(F) + M[:, r, 3]).astype(F)
                       for r in range(3)], 1)
        v = np.stack([(((M[:, r, 0] * n[:, 0]).astype(F) + (M[:, r, 1] * n[:, 1]).astype(F)).astype(F) + (M[:, r, 2] * n[:, 2]).astype(F)).astype(F) for r in range(3)], 1)
        l2 = (((v[:, 0] * v[:, 0]).astype(F) + (v[:, 1] * v[:, 1]).astype(F)).astype(F) + (v[:, 2] * v[:, 2]).astype(F)).astype(F)
        ok = (l2 > 0) & np.isfinite(l2)
        length = np.sqrt(np.where(ok, l2, F(1.0)).astype(F)).astype(F)
        on = np.where(ok[:, None], (v / length[:, None]).astype(F), v).astype(F)
    return op.reshape(verts.shape).astype(F), on.reshape(verts.shape).astype(F)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what):
    g, w = bits(got), bits(want)
    bad = np.flatnonzero((g != w).reshape(-1))
    assert g.shape == w.shape and len(bad) == 0, \
        f"{what}: {len(bad)} of {g.size} floats differ, first at {bad[:4]}: {np.asarray(got, F).reshape(-1)[bad[:4]]} against {np.asarray(want, F).reshape(-1)[bad[:4]]}"


def assert_box_contains(box, positions, what):
    """hr_skin_bounds' claim: finite, lo <= hi, and every corner inside"""
    box = np.asarray(box, F).reshape(2, 3)
    assert np.isfinite(box).all() and (box[0] <= box[1]).all(), (what, box)
    p = np.asarray(positions, F).reshape(-1, 3)
    inside = (p >= box[0]).all(1) & (p <= box[1]).all(1)
    assert inside.all(), f"{what}: {int((~inside).sum())} of {len(p)} corners outside the box {box.tolist()}, first {p[~inside][:2].tolist()}"
