"""Skinning on the GPU (include/hr_skin.h, csrc/skinning.hip): k_skin_pose against the numpy restatement (tests/skin_reference.py) as uint32 on both
entry points, and the posed buffers carried through every consumer they were made for — hr_scene_update_vertices of a flat deformable scene,
hr_scene_update_meshes of a shared one with hr_skin_bounds' box (no stream wait), the motion vectors, and a captured pose + refit."""
import numpy as np
import pytest

import helpers
import skin_cases as sc
import skin_reference as sr
from hybrid_rendering_amd import synth
from test_gpu_deformable import check_queries, cuda, scene_rays
from test_gpu_instances_shared import answers, assert_same

pytestmark = pytest.mark.gpu
F = np.float32
CASES = sc.cases()
BAR_FIRST, BAR_MESH_ID = 32, 9


@pytest.fixture(scope="module")
def sk(hr):
    from hybrid_rendering_amd import skinning
    return skinning


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


def read(skin):
    import torch
    torch.cuda.synchronize()
    return skin.positions.cpu().numpy(), skin.normals.cpu().numpy()


def check_both_entry_points(sk, ctx, arrays, matrices, mw, what):
    rp, rn = sr.pose(arrays, matrices, mw)
    skin = sk.Skin(ctx, arrays)
    for entry in ("device", "host"):
        skin.pose(sc.identity_palette(arrays["n_joints"]))        # something else in the buffers first
        if entry == "device":
            skin.pose(dev(matrices), dev(mw) if (mw is not None and len(mw)) else None)
        else:
            skin.pose(matrices, mw)
        gp, gn = read(skin)
        sr.assert_same_bits(gp, rp, f"{what}, {entry} entry point: positions")
        sr.assert_same_bits(gn, rn, f"{what}, {entry} entry point: normals")
    skin.close()
    return rp, rn


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_reference_on_every_case(sk, ctx, case):
    rp, rn = check_both_entry_points(sk, ctx, case["arrays"], case["matrices"], case["morph_weights"], case["name"])
    if case.get("identity"):
        sr.assert_same_bits(rp, case["arrays"]["verts"], "identity")
    if case.get("hostile"):
        assert np.isfinite(rp).all() and np.isfinite(rn).all()


@pytest.mark.parametrize("n_tris", [1, 7, 22, 171])
def test_size_sweep_on_both_sides_of_the_palette_cap(sk, ctx, n_tris):
    """corners 3, 21, 66 and 513 — below a wave, no multiple of 64, one past two 256-lane blocks — with n_joints 1, 2, lds_joint_cap (the palette staged
    in LDS) and lds_joint_cap + 1 (read through L2), and 0, 1 and 3 morph targets"""
    probe = sk.Skin(ctx, sc.bar(1))
    cap = probe.info()["lds_joint_cap"]
    probe.close()
    assert 64 <= cap < 65535
    for n_joints in (1, 2, cap, cap + 1):
        for n_targets in (0, 1, 3):
            arrays, mats, mw = sc.random_skin(n_tris, n_joints, n_targets, seed=1000 * n_tris + 10 * n_targets + (n_joints % 7), normal_deltas=n_targets != 1)
            check_both_entry_points(sk, ctx, arrays, mats, mw, f"{n_tris} triangles, {n_joints} joints, {n_targets} targets")


def test_a_large_skin_walks_several_passes_per_workgroup(sk, ctx):
    """above 4 workgroups of 256 corners per CU a workgroup walks several 256-corner passes behind one staged palette: 180 001 triangles are
    540 003 corners — two passes each on 256 CUs, a ragged last workgroup — on both palette paths; corner indices past 2^16 and float offsets past 2^20"""
    probe = sk.Skin(ctx, sc.bar(1))
    cap = probe.info()["lds_joint_cap"]
    probe.close()
    arrays, mats, mw = sc.random_skin(180001, cap, 1, seed=31)
    rp, rn = sr.pose(arrays, mats, mw)
    for n_joints, palette in ((cap, mats), (cap + 1, np.concatenate([mats, sc.identity_palette(1)]))):
        skin = sk.Skin(ctx, dict(arrays, n_joints=n_joints))
        skin.pose(dev(palette), dev(mw))
        gp, gn = read(skin)
        sr.assert_same_bits(gp, rp, f"{n_joints} joints: positions")
        sr.assert_same_bits(gn, rn, f"{n_joints} joints: normals")
        skin.close()


def test_both_palette_paths_give_the_same_bits(sk, ctx):
    """the same skin declared with lds_joint_cap joints and with one more (the extra joint unused): LDS-staged and L2-read palettes, equal outputs"""
    probe = sk.Skin(ctx, sc.bar(1))
    cap = probe.info()["lds_joint_cap"]
    probe.close()
    arrays, mats, mw = sc.random_skin(171, cap, 3, seed=77)
    wide = dict(arrays, n_joints=cap + 1)
    mats_wide = np.concatenate([mats, sc.identity_palette(1)])
    a, b = sk.Skin(ctx, arrays), sk.Skin(ctx, wide)
    a.pose(dev(mats), dev(mw)); b.pose(dev(mats_wide), dev(mw))
    (pa, na), (pb, nb) = read(a), read(b)
    sr.assert_same_bits(pa, pb, "positions, LDS against L2")
    sr.assert_same_bits(na, nb, "normals, LDS against L2")
    a.close(); b.close()


def test_two_host_poses_without_a_wait_in_between(sk, ctx):
    """the staging buffer: the second hr_skin_pose must not overwrite what the first one's copy still reads, and the buffers end as the second pose"""
    probe = sk.Skin(ctx, sc.bar(1))
    cap = probe.info()["lds_joint_cap"]
    probe.close()
    arrays, mats_a, mw_a = sc.random_skin(171, cap + 1, 3, seed=5)
    _, mats_b, mw_b = sc.random_skin(171, cap + 1, 3, seed=6)
    skin = sk.Skin(ctx, arrays)
    for _ in range(3):
        skin.pose(mats_a, mw_a)
        skin.pose(mats_b, mw_b)
    gp, gn = read(skin)
    rp, rn = sr.pose(arrays, mats_b, mw_b)
    sr.assert_same_bits(gp, rp, "second pose: positions")
    sr.assert_same_bits(gn, rn, "second pose: normals")
    skin.pose(mats_a, mw_a)
    gp, _ = read(skin)
    sr.assert_same_bits(gp, sr.pose(arrays, mats_a, mw_a)[0], "first pose again")
    skin.close()


def test_host_pose_refuses_non_finite_used_matrices_and_capture(sk, hr, ctx):
    import torch
    arrays = sc.bar(3)
    skin = sk.Skin(ctx, arrays)
    pal = sc.bend_palette(3, 0.2)
    skin.pose(pal)
    before = read(skin)[0]
    bad = pal.copy()
    bad[1, 5] = np.inf
    with pytest.raises(hr.HRError, match="joint 1 is not finite"):
        skin.pose(bad)
    stream, graph, scratch = torch.cuda.Stream(), torch.cuda.CUDAGraph(), torch.zeros(4, device="cuda")
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(hr.HRError, match="captur"):
            skin.pose(pal)
        scratch.add_(1.0)
    graph.replay()
    sr.assert_same_bits(read(skin)[0], before, "a refused pose enqueues nothing")
    skin.set_profiling(True)
    skin.pose(dev(pal))
    times = skin.stage_times()
    assert [t[0] for t in times] == ["skin_pose"] and times[0][1] > 0.0 and times[0][2] >= 192 * 72
    skin.close()


# ---- the consumers ----------------------------------------------------------------------------------------------------------------------------

def bar_scene_data(verts, normals):
    room = synth.cornell32()
    return synth.SceneData(verts=verts, normals=normals, tri_material=np.zeros(len(verts), np.uint32), tri_mesh_id=np.full(len(verts), BAR_MESH_ID, np.uint32),
                           materials=room.materials, name="bar")


def cornell_with_bar(verts, normals):
    room, b = synth.cornell32(), bar_scene_data(verts, normals)
    return synth.SceneData(verts=np.concatenate([room.verts, b.verts]).astype(F), normals=np.concatenate([room.normals, b.normals]).astype(F),
                           tri_material=np.concatenate([room.tri_material, b.tri_material]), tri_mesh_id=np.concatenate([room.tri_mesh_id, b.tri_mesh_id]),
                           materials=room.materials, name="cornell32_bar")


POSES = [(0.35, (0.0, 0.0, 0.0), None), (-0.5, (6.0, 2.0, -4.0), [0.8, 0.0, -0.4]), (0.8, (-8.0, 5.0, 10.0), [-1.0, 1.5, 0.6])]


def bar_with_targets():
    return sc.with_targets(sc.bar(3), 3, True, seed=12)


def test_flat_scene_end_to_end(sk, oracle, hr, ctx):
    """cornell32 with the 64-triangle bar appended: pose, update_vertices(first_tri=32) from the skin's buffers; queries equal hr.Scene over the
    numpy-skinned vertices and brute force on the ray families of tests/test_gpu_deformable.py"""
    arrays = bar_with_targets()
    g = hr.Scene(ctx, cornell_with_bar(arrays["verts"], arrays["normals"]), deformable=True)
    skin = sk.Skin(ctx, arrays)
    for i, (angle, shift, mw) in enumerate(POSES):
        pal = sc.bend_palette(3, angle, translate=shift)
        skin.pose(pal, mw)
        g.update_vertices(skin.positions, skin.normals, first_tri=BAR_FIRST)
        rp, rn = sr.pose(arrays, pal, mw)
        check_queries(hr, ctx, oracle, g, cornell_with_bar(rp, rn), f"pose {i}", seed=40 + i)
    skin.close(); g.close()


def test_shared_scene_updates_without_a_stream_wait(sk, hr, ctx):
    """the bar as one flagged mesh under two instances of synth.instanced_cornell: update_meshes with bounds = skin.bounds(...) waits for nothing,
    mesh_refit_cost reports no bound violation, answers equal a fresh shared scene over the same vertices"""
    arrays = bar_with_targets()
    isd = synth.instanced_cornell(5, seed=3)
    bar_idx = len(isd.meshes)
    isd.meshes.append(bar_scene_data(arrays["verts"], arrays["normals"]))
    isd.instances += [(synth.model_matrix(), bar_idx, 20), (synth.model_matrix((-25.0, 5.0, 20.0), (0.2, 1.0, 0.1), 0.7, 0.8), bar_idx, 21)]
    g = hr.InstancedScene(ctx, isd, shared=True, deformable=[0] * bar_idx + [1])
    skin = sk.Skin(ctx, arrays)
    for i, (angle, shift, mw) in enumerate(POSES):
        pal = sc.bend_palette(3, angle, translate=shift)
        box = skin.bounds(pal, mw)
        waits = g.update_meshes_stats()["stream_waits"]
        skin.pose(dev(pal), dev(mw))
        g.update_meshes([dict(mesh_idx=bar_idx, positions=skin.positions, normals=skin.normals, bounds=box)])
        assert g.update_meshes_stats()["stream_waits"] == waits, "bounds given: the update waits for nothing"
        assert g.mesh_refit_cost(bar_idx) > 0.0          # raises when the box given did not contain the mesh
        rp, rn = sr.pose(arrays, pal, mw)
        sr.assert_box_contains(box, rp, f"pose {i}")
        fresh_isd = synth.InstancedSceneData(meshes=isd.meshes[:bar_idx] + [bar_scene_data(rp, rn)], instances=isd.instances, materials=isd.materials)
        fresh = hr.InstancedScene(ctx, fresh_isd, shared=True)
        rays = cuda(scene_rays(fresh_isd.flatten().verts, 20000, seed=60 + i))
        a = answers(g, rays)
        assert_same(a, answers(fresh, rays), f"pose {i}: skinned shared scene against a fresh one")
        assert 0.10 <= float((a[0] != 0).mean()) <= 0.95
        fresh.close()
    skin.close(); g.close()


def test_motion_vectors_follow_the_skinned_update(sk, hr, ctx):
    """64x48, two frames, motion_begin_frame before each update: the four images equal, bit for bit, those of a second scene that got the same vertices
    uploaded from the host; texels off the bar keep the plain G-buffer's bits, texels on it carry motion in the second frame"""
    W, H = 64, 48
    arrays = bar_with_targets()
    sd0 = cornell_with_bar(arrays["verts"], arrays["normals"])
    g, gh = hr.Scene(ctx, sd0, deformable=True), hr.Scene(ctx, sd0, deformable=True)
    skin = sk.Skin(ctx, arrays)
    cams = helpers.cameras("cornell", W / H, 3, 1.0)
    keys = ("gb1", "gb2", "gb3", "depth")

    def images(d):
        return {k: np.ascontiguousarray(d[k].cpu().numpy().view(np.uint16) if d[k].element_size() == 2 else d[k].cpu().numpy()) for k in keys}

    carried = []
    for f, (angle, shift, mw) in enumerate(POSES[:2]):
        pal = sc.bend_palette(3, angle, translate=shift)
        rp, rn = sr.pose(arrays, pal, mw)
        g.motion_begin_frame(); gh.motion_begin_frame()
        skin.pose(dev(pal), dev(mw))
        g.update_vertices(skin.positions, skin.normals, first_tri=BAR_FIRST)
        gh.update_vertices(cuda(rp), cuda(rn), first_tri=BAR_FIRST)
        ubo = synth.make_ubo(cams[f + 1], cams[f], helpers.light_for("cornell", "soft"))
        a, b, plain = images(g.gbuffer(ubo, W, H, motion=True)), images(gh.gbuffer(ubo, W, H, motion=True)), images(g.gbuffer(ubo, W, H))
        for k in keys:
            assert np.array_equal(a[k], b[k]), f"frame {f}: {k} differs from the host-uploaded scene in {int((a[k] != b[k]).sum())} words"
        on_bar = (plain["gb3"].view(np.float16)[..., 2].astype(np.int64) == BAR_MESH_ID) & (plain["depth"] < 1.0)
        assert on_bar.sum() > 20 and (~on_bar).sum() > 1000, int(on_bar.sum())
        for k in keys:
            assert np.array_equal(a[k][~on_bar], plain[k][~on_bar]), f"frame {f}: {k} of a texel off the bar changed"
        carried.append(float((a["gb2"][on_bar][:, 2:] != plain["gb2"][on_bar][:, 2:]).any(axis=1).mean()))
    assert carried[1] > 0.9, carried
    skin.close(); g.close(); gh.close()


def test_captured_pose_and_refit_replay_the_rewritten_palette(sk, hr, ctx):
    """pose_device + update_vertices captured once (one linear chain); the matrix tensor is rewritten in place, the replay poses from it"""
    import torch
    arrays = bar_with_targets()
    g = hr.Scene(ctx, cornell_with_bar(arrays["verts"], arrays["normals"]), deformable=True)
    skin = sk.Skin(ctx, arrays)
    pals = [sc.bend_palette(3, a, translate=s) for a, s, _ in POSES]
    mws = [np.asarray(m if m is not None else [0.0, 0.0, 0.0], F) for _, _, m in POSES]
    pal_d, mw_d = dev(pals[0]), dev(mws[0])
    skin.pose(pal_d, mw_d)
    g.update_vertices(skin.positions, skin.normals, first_tri=BAR_FIRST)     # eager once
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        skin.pose(pal_d, mw_d)
        g.update_vertices(skin.positions, skin.normals, first_tri=BAR_FIRST)
    for i in (1, 2):
        pal_d.copy_(dev(pals[i])); mw_d.copy_(dev(mws[i]))
        graph.replay()
        rp, rn = sr.pose(arrays, pals[i], mws[i])
        gp, gn = read(skin)
        sr.assert_same_bits(gp, rp, f"replay {i}: positions")
        sr.assert_same_bits(gn, rn, f"replay {i}: normals")
        fresh = hr.Scene(ctx, cornell_with_bar(rp, rn))
        rays = cuda(scene_rays(cornell_with_bar(rp, rn).verts, 20000, seed=80 + i))
        assert_same(answers(g, rays), answers(fresh, rays), f"replay {i}: the refitted scene against a fresh one")
        fresh.close()
    skin.close(); g.close()
