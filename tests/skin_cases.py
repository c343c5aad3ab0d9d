"""The case table of the skinning tests (tests/test_skin_cases.py on the host, tests/test_gpu_skin.py on the GPU): a bending bar and the edges of
include/hr_skin.h's contract.  A case is a dict: name, arrays (what skinning.SkinArrays and skin_reference.pose take), matrices [n_joints,16]
float32 column-major, morph_weights (None or [n_targets] float32), and flags the tests read (identity: positions keep the rest bits;
zero_normal: some normal comes out exactly zero; hostile: a matrix no live slot names is not finite)."""
import math

import numpy as np

F = np.float32
BAR_AT, BAR_LENGTH, BAR_HALF, BAR_SEGMENTS = (50.0, 12.0, 50.0), 40.0, 4.0, 8


def colmajor(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16), F)


def trs(translate=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0), angle=0.0, scale=1.0, pivot=(0.0, 0.0, 0.0)):
    """4x4 float64: T(translate) T(pivot) R(axis, angle) S(scale) T(-pivot)"""
    a = np.asarray(axis, np.float64)
    x, y, z = a / max(np.linalg.norm(a), 1e-30)
    c, s = math.cos(angle), math.sin(angle)
    R = np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                  [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                  [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])
    M = np.eye(4)
    M[:3, :3] = R * np.broadcast_to(np.asarray(scale, np.float64), (3,))[None, :]
    P, Q, T = np.eye(4), np.eye(4), np.eye(4)
    P[:3, 3], Q[:3, 3], T[:3, 3] = pivot, -np.asarray(pivot, np.float64), translate
    return T @ P @ M @ Q


def identity_palette(n_joints):
    return np.ascontiguousarray(np.tile(colmajor(np.eye(4)), (n_joints, 1)), F)


def bar(n_joints=3):
    """A 4-sided prism along +y, 8 segments, 64 triangles, smooth weights over joints spread along its length (slots 0 and 1 live)."""
    x0, y0, z0 = BAR_AT
    h = BAR_HALF
    ring = [(-h, -h), (h, -h), (h, h), (-h, h)]
    side_n = [(0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0)]
    verts, normals, u_of = [], [], []
    for s in range(BAR_SEGMENTS):
        ya, yb = y0 + BAR_LENGTH * s / BAR_SEGMENTS, y0 + BAR_LENGTH * (s + 1) / BAR_SEGMENTS
        ua, ub = s / BAR_SEGMENTS, (s + 1) / BAR_SEGMENTS
        for q in range(4):
            (ax, az), (bx, bz) = ring[q], ring[(q + 1) % 4]
            A, B, Cc, D = (x0 + ax, ya, z0 + az), (x0 + bx, ya, z0 + bz), (x0 + bx, yb, z0 + bz), (x0 + ax, yb, z0 + az)
            verts += [[A, Cc, B], [A, D, Cc]]
            u_of += [[ua, ub, ua], [ua, ub, ub]]
            normals += [[side_n[q]] * 3, [side_n[q]] * 3]
    verts, normals, u = np.asarray(verts, F), np.asarray(normals, F), np.asarray(u_of, np.float64)
    joints, weights = np.zeros((64, 3, 4), np.uint16), np.zeros((64, 3, 4), np.float64)
    f = u * max(n_joints - 1, 1) if n_joints > 1 else np.zeros_like(u)
    j0 = np.minimum(np.floor(f), max(n_joints - 2, 0)).astype(np.int64)
    frac = f - j0
    joints[..., 0], joints[..., 1] = j0, np.minimum(j0 + 1, n_joints - 1)
    weights[..., 0], weights[..., 1] = 1.0 - frac, frac
    if n_joints == 1:
        weights[..., 0], weights[..., 1] = 1.0, 0.0
    weights /= weights.sum(-1, keepdims=True)
    return dict(verts=verts, normals=normals, joints=joints, weights=weights.astype(F), n_joints=n_joints, target_positions=None, target_normals=None)


def bar_pivots(n_joints):
    x0, y0, z0 = BAR_AT
    return [(x0, y0 + BAR_LENGTH * j / max(n_joints - 1, 1), z0) for j in range(n_joints)]


def bend_palette(n_joints, angle, translate=(0.0, 0.0, 0.0), scale=1.0, axis=(0.0, 0.0, 1.0)):
    """joint j turns by j * angle about `axis` through its pivot on the bar"""
    return np.stack([colmajor(trs(translate, axis, angle * j, scale, pivot)) for j, pivot in enumerate(bar_pivots(n_joints))])


def with_targets(arrays, n_targets, normal_deltas, seed=5):
    rng = np.random.RandomState(seed)
    a = dict(arrays)
    n = a["verts"].shape[0]
    a["target_positions"] = rng.uniform(-1.5, 1.5, (n_targets, n, 3, 3)).astype(F) if n_targets else None
    a["target_normals"] = rng.uniform(-0.3, 0.3, (n_targets, n, 3, 3)).astype(F) if (n_targets and normal_deltas) else None
    return a


def move_slots(arrays, order):
    """slot k of the result is slot order[k] of `arrays` (-1: an empty slot, weight +0, joint 0)"""
    a = dict(arrays)
    j, w = np.zeros_like(arrays["joints"]), np.zeros_like(arrays["weights"])
    for k, src in enumerate(order):
        if src >= 0:
            j[..., k], w[..., k] = arrays["joints"][..., src], arrays["weights"][..., src]
    a["joints"], a["weights"] = j, w
    return a


def case(name, arrays, matrices, morph_weights=None, **flags):
    mw = None if morph_weights is None else np.asarray(morph_weights, F)
    return dict(name=name, arrays=arrays, matrices=np.ascontiguousarray(matrices, F), morph_weights=mw, **flags)


def cases():
    out = []
    b2, b3 = bar(2), bar(3)
    out.append(case("bar_2_joints", b2, bend_palette(2, 0.5)))
    out.append(case("bar_3_joints", b3, bend_palette(3, 0.35, translate=(1.5, -2.0, 0.25), scale=(1.1, 0.9, 1.25))))

    one = bar(1)
    out.append(case("slot_3_only", move_slots(one, (-1, -1, -1, 0)), bend_palette(1, 0.0, translate=(3.0, 1.0, -2.0), scale=1.5)))
    out.append(case("slots_1_and_2", move_slots(b3, (-1, 0, 1, -1)), bend_palette(3, -0.4)))

    neg = move_slots(b3, (0, -1, 1, -1))
    neg["weights"][..., 1] = F(-0.0)
    neg["weights"][::2, :, 3] = F(-0.0)
    out.append(case("negative_zero_weight", neg, bend_palette(3, 0.3)))

    # joint 3 is named by zero-weight slots only, and a zero-weight slot may name no joint of the skin at all: neither is ever read
    hostile = move_slots(b3, (0, 1, -1, -1))
    hostile["n_joints"] = 5
    hostile["joints"][..., 2], hostile["joints"][..., 3] = 3, 65535
    hostile["joints"][1::2, :, 3] = 4
    pal = np.concatenate([bend_palette(3, 0.25), identity_palette(2)])
    pal[3] = [np.inf, 1.0, np.nan, 0.0, -np.inf, np.nan, 2.0, 0.0, np.nan, np.inf, 1.0, 0.0, np.inf, np.nan, -np.inf, 1.0]
    pal[4] = np.nan
    out.append(case("zero_weight_slot_names_a_non_finite_joint", hostile, pal, hostile=True))

    out.append(case("identity_one_influence", one, identity_palette(1), identity=True))
    out.append(case("identity_one_influence_slot_2", move_slots(one, (-1, -1, 0, -1)), identity_palette(1), identity=True))

    # halves of the identity and of a half turn about z: mat3 of the blend is diag(0, 0, 1), the side normals (+-x, +-z) with no z go to zero
    half = bar(2)
    half["weights"][..., 0], half["weights"][..., 1] = F(0.5), F(0.5)
    half["joints"][..., 0], half["joints"][..., 1] = 0, 1
    out.append(case("degenerate_blend_zero_normal", half, np.stack([colmajor(np.eye(4)), colmajor(np.diag([-1.0, -1.0, 1.0, 1.0]))]), zero_normal=True))

    out.append(case("translations_of_1e6", b3, bend_palette(3, 0.2, translate=(1.0e6, -1.0e6, 1.0e6))))

    out.append(case("morph_0_targets_weights_given", with_targets(b3, 0, False), bend_palette(3, 0.3), morph_weights=np.zeros(0, F)))
    out.append(case("morph_1_target", with_targets(b3, 1, True), bend_palette(3, 0.3), morph_weights=[0.75]))
    out.append(case("morph_1_target_weight_zero", with_targets(b3, 1, True), bend_palette(3, 0.3), morph_weights=[0.0]))
    out.append(case("morph_3_targets_one_zero_normal_deltas", with_targets(b3, 3, True), bend_palette(3, -0.3), morph_weights=[1.25, 0.0, -0.5]))
    out.append(case("morph_3_targets_one_zero_no_normal_deltas", with_targets(b3, 3, False), bend_palette(3, -0.3), morph_weights=[-1.0, 2.0, 0.0]))
    out.append(case("morph_3_targets_no_weights", with_targets(b3, 3, True), bend_palette(3, -0.3), morph_weights=None))
    return out


def random_skin(n_tris, n_joints, n_targets, seed, normal_deltas=True):
    """(arrays, matrices, morph_weights): random corners, four slots of which about 40 % are empty (slot 0 is refilled where all four were),
    weights normalised in float64, rigid-plus-scale matrices; morph weights with one exact zero when there are three targets"""
    rng = np.random.RandomState(seed)
    verts = rng.uniform(-10.0, 10.0, (n_tris, 3, 3)).astype(F)
    nrm = rng.normal(size=(n_tris, 3, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    joints = rng.randint(0, n_joints, (n_tris, 3, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, (n_tris, 3, 4))
    w[rng.uniform(size=w.shape) < 0.4] = 0.0
    dead = w.sum(-1) == 0
    w[..., 0][dead] = 1.0
    w /= w.sum(-1, keepdims=True)
    arrays = dict(verts=verts, normals=nrm, joints=joints, weights=w.astype(F), n_joints=n_joints, target_positions=None, target_normals=None)
    arrays = with_targets(arrays, n_targets, normal_deltas, seed + 1)
    mats = np.stack([colmajor(trs(rng.uniform(-20, 20, 3), rng.uniform(-1, 1, 3), rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 2.0, 3))) for _ in range(n_joints)])
    mw = None
    if n_targets:
        mw = rng.uniform(-1.0, 2.0, n_targets).astype(F)
        if n_targets >= 3:
            mw[1] = 0.0
    return arrays, mats, mw
