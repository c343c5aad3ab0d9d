"""assets.load_gltf_skinned and SkinnedMesh.pose without a GPU: a two-joint bar with one morph target and one animation (a LINEAR rotation track, a
STEP translation track, a weights track), written here as a .gltf with base64 buffers, loads to the arrays the test wrote; the sampled palettes
equal hand-built matrices; what the loader does not support raises a ValueError that names it."""
import base64
import copy
import json
import math

import numpy as np
import pytest

import skin_reference as sr
from hybrid_rendering_amd import assets

F = np.float32
FLOAT, UBYTE, USHORT = 5126, 5121, 5123


class Builder:
    def __init__(self):
        self.blob, self.views, self.accessors = b"", [], []

    def add(self, a, comp, typ, normalized=False):
        a = np.ascontiguousarray(a)
        self.blob += b"\0" * (-len(self.blob) % 4)
        self.views.append(dict(buffer=0, byteOffset=len(self.blob), byteLength=a.nbytes))
        self.blob += a.tobytes()
        acc = dict(bufferView=len(self.views) - 1, componentType=comp, count=int(a.shape[0]), type=typ)
        if normalized:
            acc["normalized"] = True
        self.accessors.append(acc)
        return len(self.accessors) - 1


POS = np.array([[-1, 0, 0], [1, 0, 0], [-1, 1, 0], [1, 1, 0], [-1, 2, 0], [1, 2, 0]], F)
NRM = np.tile(np.array([[0, 0, 1]], F), (6, 1))
IDX = np.array([0, 1, 2, 2, 1, 3, 2, 3, 4, 4, 3, 5], np.uint16)
JOINTS = np.array([[0, 1, 0, 0]] * 6, np.uint8)
WEIGHTS = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.5, 0.5, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]], F)
DPOS = np.array([[0, 0, 0.5]] * 6, F) * np.arange(6, dtype=F)[:, None]
DNRM = np.array([[0.1, 0, 0]] * 6, F)
TIMES = np.array([0.0, 1.0, 2.0], F)


def quat_z(angle):
    return [0.0, 0.0, math.sin(angle / 2), math.cos(angle / 2)]


ROT = np.array([quat_z(0.0), quat_z(math.pi / 2), quat_z(2.0)], F)
TRANS = np.array([[0, 0, 0], [1, 0, 0], [2, 0.5, 0]], F)
MORPH = np.array([0.0, 0.5, 1.0], F)


def document(weights=WEIGHTS, weights_comp=FLOAT, joints=JOINTS, joints_comp=UBYTE):
    b = Builder()
    normalized = weights_comp != FLOAT
    a = dict(pos=b.add(POS, FLOAT, "VEC3"), nrm=b.add(NRM, FLOAT, "VEC3"), idx=b.add(IDX, USHORT, "SCALAR"), j=b.add(joints, joints_comp, "VEC4"),
             w=b.add(weights, weights_comp, "VEC4", normalized), dp=b.add(DPOS, FLOAT, "VEC3"), dn=b.add(DNRM, FLOAT, "VEC3"),
             ibm=b.add(np.stack([np.eye(4, dtype=F).T.reshape(16), translate(0, -1, 0).T.reshape(16).astype(F)]), FLOAT, "MAT4"),
             t=b.add(TIMES, FLOAT, "SCALAR"), rot=b.add(ROT, FLOAT, "VEC4"), tr=b.add(TRANS, FLOAT, "VEC3"), mw=b.add(MORPH, FLOAT, "SCALAR"))
    b.accessors[a["pos"]].update(min=POS.min(0).tolist(), max=POS.max(0).tolist())
    return dict(
        asset=dict(version="2.0"), scene=0, scenes=[dict(nodes=[0, 1])],
        nodes=[dict(mesh=0, skin=0, translation=[5.0, 5.0, 5.0]), dict(name="root", children=[2]), dict(name="tip", translation=[0.0, 1.0, 0.0])],
        meshes=[dict(name="bar", weights=[0.25], primitives=[dict(attributes=dict(POSITION=a["pos"], NORMAL=a["nrm"], JOINTS_0=a["j"], WEIGHTS_0=a["w"]), indices=a["idx"],
                                                                  targets=[dict(POSITION=a["dp"], NORMAL=a["dn"])])])],
        skins=[dict(joints=[1, 2], inverseBindMatrices=a["ibm"])],
        animations=[dict(name="bend", samplers=[dict(input=a["t"], output=a["rot"], interpolation="LINEAR"), dict(input=a["t"], output=a["tr"], interpolation="STEP"),
                                                dict(input=a["t"], output=a["mw"])],
                         channels=[dict(sampler=0, target=dict(node=2, path="rotation")), dict(sampler=1, target=dict(node=1, path="translation")),
                                   dict(sampler=2, target=dict(node=0, path="weights"))])],
        buffers=[dict(byteLength=len(b.blob), uri="data:application/octet-stream;base64," + base64.b64encode(b.blob).decode())],
        bufferViews=b.views, accessors=b.accessors)


def translate(x, y, z):
    M = np.eye(4)
    M[:3, 3] = (x, y, z)
    return M


def rot_z(angle):
    M = np.eye(4)
    c, s = math.cos(angle), math.sin(angle)
    M[:2, :2] = [[c, -s], [s, c]]
    return M


def palette(tr, angle, scale):
    """the two joint matrices by hand: root = T(tr), tip = root T(0, 1, 0) Rz(angle); times the inverse binds I and T(0, -1, 0); rows times scale"""
    root = translate(*tr)
    tip = root @ translate(0, 1, 0) @ rot_z(angle)
    out = []
    for M in (root, tip @ translate(0, -1, 0)):
        M = M.copy()
        M[:3, :] *= scale
        out.append(M.T.reshape(16))
    return np.asarray(out, F)


def write(tmp_path, doc, name="bar.gltf"):
    p = tmp_path / name
    p.write_text(json.dumps(doc))
    return str(p)


def test_the_bar_loads_to_the_arrays_the_test_wrote(tmp_path):
    m = assets.load_gltf_skinned(write(tmp_path, document()), scale=2.0)
    tri = IDX.reshape(-1, 3).astype(np.int64)
    assert m.rest.n_tris == 4 and m.n_joints == 2 and m.n_targets == 1
    assert np.array_equal(m.rest.verts, POS[tri]) and np.array_equal(m.rest.normals, NRM[tri])     # skin space: the node's translation is ignored
    assert m.joints.dtype == np.uint16 and np.array_equal(m.joints, JOINTS[tri].astype(np.uint16))
    assert m.weights.dtype == F and np.array_equal(m.weights, WEIGHTS[tri])
    assert np.array_equal(m.target_positions, DPOS[tri][None]) and np.array_equal(m.target_normals, DNRM[tri][None])
    assert m.default_morph_weights.tolist() == [0.25]
    assert m.joint_nodes == [1, 2] and m.parents == [-1, 0] and m.node_parent == [-1, -1, 1]
    assert np.array_equal(m.inverse_bind[1], translate(0, -1, 0)) and np.array_equal(m.inverse_bind[0], np.eye(4))
    assert list(m.animations) == ["bend"] and m.duration("bend") == 2.0
    rest_pal, rest_mw = m.pose(None)
    assert np.allclose(rest_pal, palette((0, 0, 0), 0.0, 2.0), atol=1e-6) and rest_mw.tolist() == [0.25]
    # the plain loaders stay as they are: they see the mesh and drop the skin
    assert assets.load_gltf(write(tmp_path, document())).n_tris == 4


def test_pose_at_keyframes_mid_intervals_and_past_the_ends(tmp_path):
    m = assets.load_gltf_skinned(write(tmp_path, document()), scale=2.0)
    angles = [0.0, math.pi / 2, 2.0]
    for k, t in enumerate(TIMES):
        pal, mw = m.pose("bend", float(t))
        assert pal.shape == (2, 16) and pal.dtype == F
        assert np.allclose(pal, palette(TRANS[k], angles[k], 2.0), atol=2e-6), (k, pal)
        assert np.allclose(mw, [MORPH[k]], atol=1e-7)
    # mid-interval: the slerp of two rotations about one axis is the mean angle, the STEP track holds the earlier key, the weights go linearly
    pal, mw = m.pose("bend", 0.5)
    assert np.allclose(pal, palette(TRANS[0], math.pi / 4, 2.0), atol=2e-6) and np.allclose(mw, [0.25], atol=1e-7)
    pal, mw = m.pose("bend", 1.75)
    assert np.allclose(pal, palette(TRANS[1], math.pi / 2 + 0.75 * (2.0 - math.pi / 2), 2.0), atol=2e-6) and np.allclose(mw, [0.875], atol=1e-7)
    # t is clamped to the track; animations go by index too
    for t, k in ((-3.0, 0), (7.5, 2)):
        pal, mw = m.pose(0, t)
        assert np.allclose(pal, palette(TRANS[k], angles[k], 2.0), atol=2e-6) and np.allclose(mw, [MORPH[k]], atol=1e-7)


def test_integer_joints_and_normalised_weights(tmp_path):
    """uint16 joints; uint8 and uint16 normalised weights whose integer sums are not 255 / 65535: each vertex is normalised to 1 in float64"""
    tri = IDX.reshape(-1, 3).astype(np.int64)
    for comp, top, dt in ((UBYTE, 255, np.uint8), (USHORT, 65535, np.uint16)):
        w = np.round(WEIGHTS.astype(np.float64) * top).astype(dt)
        w[2] = [top // 3, top // 2, 0, 0]
        m = assets.load_gltf_skinned(write(tmp_path, document(weights=w, weights_comp=comp, joints=JOINTS.astype(np.uint16), joints_comp=USHORT)))
        want = w.astype(np.float64) / top
        want = (want / want.sum(1, keepdims=True)).astype(F)
        assert np.array_equal(m.weights, want[tri]) and np.array_equal(m.joints, JOINTS[tri].astype(np.uint16))
        assert np.abs(m.weights.astype(np.float64).sum(-1) - 1.0).max() <= 2.0 ** -23


def test_the_loaded_mesh_feeds_the_host_restatement(tmp_path):
    from hybrid_rendering_amd import build as hb, skinning
    hb.build()
    m = assets.load_gltf_skinned(write(tmp_path, document()), scale=1.5)
    pal, mw = m.pose("bend", 1.25)
    a = skinning.SkinArrays(m)
    assert (a.n_tris, a.n_joints, a.n_targets) == (4, 2, 1) and skinning.check_desc(m) == 0
    hp, hn = skinning.pose_host(m, pal, mw)
    arrays = dict(verts=m.rest.verts, normals=m.rest.normals, joints=m.joints, weights=m.weights, target_positions=m.target_positions, target_normals=m.target_normals)
    rp, rn = sr.pose(arrays, pal, mw)
    sr.assert_same_bits(hp, rp, "positions")
    sr.assert_same_bits(hn, rn, "normals")
    # against float64 by hand: the vertex at the root end follows the root joint alone
    want = 1.5 * (POS[0].astype(np.float64) + mw[0] * DPOS[0] + TRANS[1])
    assert np.allclose(hp[0, 0], want, atol=1e-5)


def test_unsupported_features_raise_value_errors_that_name_the_cause(tmp_path):
    doc = document()
    cubic = copy.deepcopy(doc)
    cubic["animations"][0]["samplers"][0]["interpolation"] = "CUBICSPLINE"
    with pytest.raises(ValueError, match="CUBICSPLINE"):
        assets.load_gltf_skinned(write(tmp_path, cubic))
    more = copy.deepcopy(doc)
    at = more["meshes"][0]["primitives"][0]["attributes"]
    at["JOINTS_1"], at["WEIGHTS_1"] = at["JOINTS_0"], at["WEIGHTS_0"]
    with pytest.raises(ValueError, match="JOINTS_1"):
        assets.load_gltf_skinned(write(tmp_path, more))
    sparse = copy.deepcopy(doc)
    sparse["accessors"][doc["meshes"][0]["primitives"][0]["targets"][0]["POSITION"]]["sparse"] = dict(count=1, indices=dict(bufferView=0, componentType=UBYTE), values=dict(bufferView=0))
    with pytest.raises(ValueError, match="sparse"):
        assets.load_gltf_skinned(write(tmp_path, sparse))
    plain = copy.deepcopy(doc)
    del plain["nodes"][0]["skin"]
    with pytest.raises(ValueError, match="skin"):
        assets.load_gltf_skinned(write(tmp_path, plain))
