"""hr_scene_update_instances_device on the GPU (csrc/instances_shared_update.hip): a shared instanced scene updated from matrices in DEVICE
memory.  The kernels run the host path's arithmetic (csrc/instance_math.h, one body for both), so nothing here has a tolerance but the cost
ratio: records, top-level nodes, bounds, pad and every answer equal those of hr_scene_update_instances on a twin scene bit for bit.

The single-launch limit of the top-level refit is 1024 NODES (the file header of instances_shared_update.hip).  A top level over I instances has
N nodes with (I - 1) / 7 <= N <= I - 1 (every node holds 2 to 8 children, I + N - 1 children in all), so 1025 instances are refitted in one
launch and 7201 are not, whatever the SAH decides; the launch counts below confirm on which side each size falls.  3301 instances (the SAH
gives about 0.28 nodes per instance here) land between 513 and 1024 nodes: the one-workgroup kernel at its full 1024 lanes."""
import numpy as np
import pytest

import helpers
import shared_deform_cases as sc
from hybrid_rendering_amd import synth, synth_env
from test_gpu_instances import _mats, _rays
from test_gpu_instances_shared import answers, assert_same, hostile_instances
from test_gpu_instances_shared_deform import entry
from test_gpu_shared_passes import Passes, Rig, assert_equal_snapshots, gbuffer_np, mirrors

pytestmark = pytest.mark.gpu

LAUNCHES_SMALL = 2          # instances_shared_update.hip kLaunchesSmall: the record kernel, then the whole top level in one workgroup
ONE_LAUNCH_NODES = 1024     # ... kOneLaunchNodes


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def info_bounds(info):
    return np.array(list(info.bounds_lo) + list(info.bounds_hi), np.float32)


def state(g):
    """(records, top-level nodes, bounds + pad) of a shared scene"""
    info = g.refresh_info()
    return g.read_records(), g.read_bvh()[0][:len(g.isd.instances)], (list(info.bounds_lo), list(info.bounds_hi), info.box_pad)


def assert_same_state(a, b, what):
    (ra, na, ia), (rb, nb, ib) = state(a), state(b)
    assert np.array_equal(ra, rb), f"{what}: records differ in rows {np.flatnonzero((ra != rb).any(1))[:8]}"
    assert np.array_equal(na, nb), f"{what}: top-level nodes differ in slots {np.flatnonzero((na != nb).any(1))[:8]}"
    assert ia == ib, f"{what}: bounds / pad {ia} against {ib}"


# ---- the top level's half-area sum, restated in numpy from what the scene reads back -----------------------------------------------------------
def instance_boxes_np(isd, mats):
    """csrc/instance_math.h world_box: the eight corners of the mesh's bounds in fp64, widened by 1e-6 of their magnitude, rounded outward to fp32"""
    out = np.zeros((len(mats), 6), np.float32)
    for i, ((_, k, _), m) in enumerate(zip(isd.instances, np.asarray(mats, np.float32).reshape(-1, 16))):
        m = m.astype(np.float64)
        if isd.meshes[k].n_tris == 0:
            l = h = m[12:15]
        else:
            lo, hi = [b.astype(np.float64) for b in isd.meshes[k].bounds()]
            l, h = np.full(3, 1e300), np.full(3, -1e300)
            for c in range(8):
                p = [(hi if (c >> a) & 1 else lo)[a] for a in range(3)]
                v = m[0:3] * p[0] + m[4:7] * p[1] + m[8:11] * p[2] + m[12:15]
                e = 1e-6 * (np.abs(m[0:3] * p[0]) + np.abs(m[4:7] * p[1]) + np.abs(m[8:11] * p[2]) + np.abs(m[12:15]))
                l, h = np.minimum(l, v - e), np.maximum(h, v + e)
        lo32, hi32 = l.astype(np.float32), h.astype(np.float32)
        lo32 = np.where(lo32.astype(np.float64) > l, np.nextafter(lo32, np.float32(-np.inf)), lo32)
        hi32 = np.where(hi32.astype(np.float64) < h, np.nextafter(hi32, np.float32(np.inf)), hi32)
        out[i, :3], out[i, 3:] = lo32, hi32
    return out


def top_area_np(isd, mats, nodes, records, pad):
    """sum over the top level's nodes of the half area of the box of their children (leaves: instance box -+ pad in fp32), topology from the nodes"""
    boxes = instance_boxes_np(isd, mats)
    inst_of_leaf = records[:, 140:144].copy().view(np.uint32)[:, 0]
    pad = np.float32(pad)
    kids, order, at = {}, [0], 0
    while at < len(order):
        n = nodes[order[at]]
        n_int, nc = int(n[15]) & 15, int(n[15]) >> 4
        child_base, leaf_base = int(n[16:20].copy().view(np.uint32)[0]), int(n[20:24].copy().view(np.uint32)[0])
        kids[order[at]] = ([child_base + c for c in range(n_int)], [leaf_base + j for j in range(nc - n_int)])
        order += kids[order[at]][0]
        at += 1
    box, areas = {}, []
    for slot in reversed(order):
        lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for c in kids[slot][0]:
            lo, hi = np.minimum(lo, box[c][0]), np.maximum(hi, box[c][1])
        for l in kids[slot][1]:
            b = boxes[inst_of_leaf[l]]
            lo, hi = np.minimum(lo, b[:3] - pad), np.maximum(hi, b[3:] + pad)
        box[slot] = (lo, hi)
        d = hi.astype(np.float64) - lo.astype(np.float64)
        areas.append(d[0] * d[1] + d[1] * d[2] + d[2] * d[0])
    return float(np.sum(np.array(areas, np.float64))), len(order)


# ---- 1. bits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boxes,seed", [(5, 3), (70, 9), (600, 4), (1024, 6), (3300, 5), (7200, 7)])
def test_records_nodes_and_bounds_equal_the_host_path(hr, ctx, n_boxes, seed):
    """frames 0, 1, 2, 7: scene A takes update(), twin B update_device() with measured bounds, twin C update_device() with A's bounds given —
    records, top-level nodes, bounds and pad byte-equal; given bounds cost no stream wait; 2 launches per update up to 1024 top-level nodes"""
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    a, b, c = [hr.InstancedScene(ctx, isd, shared=True) for _ in range(3)]
    rebuilds = a.top_level_rebuilds
    for f in (0, 1, 2, 7):
        mats = _mats(isd, n_boxes, seed, f)
        a.update(mats)
        assert a.top_level_rebuilds == rebuilds, f"frame {f}: the host path re-built its top level, the topologies diverge"
        before = b.device_update_stats()
        b.update_device(cuda(mats), bounds=None)
        after = b.device_update_stats()
        assert after["stream_waits"] == before["stream_waits"] + 1, "measured bounds: ONE wait"
        assert_same_state(a, b, f"frame {f}, measured bounds")
        before_c = c.device_update_stats()
        c.update_device(cuda(mats), bounds=info_bounds(a.refresh_info()).reshape(2, 3))
        after_c = c.device_update_stats()
        assert after_c["stream_waits"] == before_c["stream_waits"], "given bounds: no wait"
        assert_same_state(a, c, f"frame {f}, given bounds")
        st = c.device_update_status()
        assert st["rejected_instances"] == 0 and st["bounds_violated"] == 0, st
        used = int((c.read_bvh()[0][:n_boxes + 1, 15] != 0).sum())
        grew = after_c["launches"] - before_c["launches"]
        print(f"{n_boxes + 1} instances, frame {f}: {used} top-level nodes, {grew} launches, cost ratio {st['top_cost_ratio']:.4f}")
        if n_boxes + 1 <= ONE_LAUNCH_NODES + 1:
            assert used <= ONE_LAUNCH_NODES and grew == LAUNCHES_SMALL and after["launches"] - before["launches"] == LAUNCHES_SMALL
        if n_boxes == 3300:   # the full-width configuration of the one-workgroup kernel: 1024 lanes, 16 waves, 32 KiB of LDS
            assert ONE_LAUNCH_NODES // 2 < used <= ONE_LAUNCH_NODES and grew == LAUNCHES_SMALL, (used, grew)
        if n_boxes + 1 >= 7 * ONE_LAUNCH_NODES + 2:
            assert used > ONE_LAUNCH_NODES and grew > LAUNCHES_SMALL, "the per-depth path"
    for g in (a, b, c):
        g.close()


# ---- 2. answers --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boxes,seed", [(5, 3), (70, 9), (600, 4)])
def test_answers_equal_the_host_updated_and_the_flattened_scene(hr, ctx, n_boxes, seed):
    """40 000 rays after every device update, frames 90 and 91 included: there the host path re-builds its top level and the device path does
    not, so the answers must not depend on the topology.  The cost ratio the device reports equals the numpy restatement over B's own nodes:
    a reordered fp64 sum over at most a few hundred nodes stays within 1e-9 relative, and the API hands the ratio out as an fp32 (2^-24)."""
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    a, b = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
    top = n_boxes + 1
    area_at_build, _ = top_area_np(isd, isd.matrices(), b.read_bvh()[0][:top], b.read_records(), b.refresh_info().box_pad)
    rd = cuda(_rays(40000, seed))
    host_rebuilds = a.top_level_rebuilds
    for f in (0, 1, 2, 7, 90, 91):
        mats = _mats(isd, n_boxes, seed, f)
        a.update(mats)
        b.update_device(cuda(mats))
        assert b.top_level_rebuilds == 0
        gf = hr.Scene(ctx, isd.flatten(mats))
        got = answers(b, rd)
        assert_same(got, answers(a, rd), f"frame {f}: device-updated against host-updated")
        assert_same(got, answers(gf, rd), f"frame {f}: device-updated against the flattened scene")
        gf.close()
        assert 0.05 < got[0].mean() < 0.999
        st = b.device_update_status()
        area, used = top_area_np(isd, mats, b.read_bvh()[0][:top], b.read_records(), b.refresh_info().box_pad)
        want = area / area_at_build
        print(f"{top} instances, frame {f}: {used} nodes, cost ratio {st['top_cost_ratio']!r} (numpy {want!r}), host re-builds {a.top_level_rebuilds - host_rebuilds}")
        # 1e-9 relative is the bound on the fp64 sums (the device's fixed order against numpy's); the C ABI hands the ratio out as a `float`,
        # whose rounding adds up to 2^-24 relative — the only reason this bound is wider than 1e-9
        assert abs(st["top_cost_ratio"] - want) <= want * (2.0 ** -24 + 1e-9), (st, want)
        if f >= 90:
            assert st["top_cost_ratio"] > 1.0
    if n_boxes > 5:
        assert a.top_level_rebuilds > host_rebuilds, "frames 90 / 91 are there because the host path re-builds on them"
    a.close(); b.close()


# ---- 3. hostile matrices -----------------------------------------------------------------------------------------------------------------------
def test_hostile_matrices_make_the_host_paths_records(hr, ctx):
    """zero scale, 1e-4 and 1e4 scales, a shear, condition 1e6 / 9e6 / 1.1e7, an empty mesh: the records (flags = 1 included) and the nodes are
    the host path's, and the answers the flattened scene's"""
    isd = hostile_instances(synth.instanced_cornell(4, seed=8))
    a, b = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
    rd = cuda(_rays(20000, 12))
    mats = isd.matrices()
    for step in (1, 2):
        mats = mats.copy()
        mats[1:5, 12:15] += np.float32(3.5 * step)
        mats[8, 12:15] += np.float32(-500.0 * step)
        mats[-3:, 12:15] += np.float32(0.25 * step)          # the ill-conditioned ones move too: their records are rewritten on the device
        mats[6, 0:3] *= np.float32(1.0 + step)                # the plane stays a plane
        a.update(mats)
        b.update_device(cuda(mats))
        assert_same_state(a, b, f"step {step}")
        flags = b.read_records()[:, 116:120].copy().view(np.uint32)[:, 0]
        assert flags.sum() >= 3, "zero scales and the matrix beyond condition 1e7 walk without culling"
        gf = hr.Scene(ctx, isd.flatten(mats))
        assert_same(answers(b, rd), answers(gf, rd), f"step {step}: against the flattened scene")
        gf.close()
    a.close(); b.close()


# ---- 4. non-finite matrices --------------------------------------------------------------------------------------------------------------------
def test_non_finite_matrices_keep_their_instances_as_they_were(hr, ctx):
    n_boxes, seed = 70, 9
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    a, b = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
    m1, m2 = _mats(isd, n_boxes, seed, 1), _mats(isd, n_boxes, seed, 2)
    a.update(m1); b.update_device(cuda(m1))
    rec1 = b.read_records()
    leaf_of = {int(i): l for l, i in enumerate(rec1[:, 140:144].copy().view(np.uint32)[:, 0])}
    bad = m2.copy()
    nan_i, inf_i = 4, 40                                       # boxes 3 and 39: instances that move between the frames
    assert not np.array_equal(m1[nan_i], m2[nan_i]) and not np.array_equal(m1[inf_i], m2[inf_i])
    bad[nan_i, 5] = np.nan; bad[inf_i, 13] = np.inf
    b.update_device(cuda(bad))
    assert b.device_update_status()["rejected_instances"] == 2
    kept = m2.copy()
    kept[nan_i], kept[inf_i] = m1[nan_i], m1[inf_i]
    a.update(kept)
    rec2 = b.read_records()
    for i in (nan_i, inf_i):
        assert np.array_equal(rec2[leaf_of[i]], rec1[leaf_of[i]]), f"instance {i} keeps its record"
    changed = (rec2 != rec1).any(1)
    moving = [leaf_of[i] for i in range(n_boxes + 1) if not np.array_equal(m1[i], m2[i]) and i not in (nan_i, inf_i)]
    assert changed[moving].all() and int(changed.sum()) == len(moving), "every other record is updated, and no more"
    assert_same_state(a, b, "after the rejected matrices")    # the boxes of the two are the old ones: the top level equals the host's
    rd = cuda(_rays(40000, seed))
    assert_same(answers(b, rd), answers(a, rd), "queries against the host scene in which the two kept their matrices")
    b.update_device(cuda(m2))
    assert b.device_update_status()["rejected_instances"] == 0
    a.close(); b.close()


# ---- 5. bounds ---------------------------------------------------------------------------------------------------------------------------------
def test_bounds_that_cut_an_instance_off_are_reported(hr, ctx):
    import torch
    n_boxes, seed = 70, 9
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    a, b = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
    mats = _mats(isd, n_boxes, seed, 1).copy()
    mats[5, 12] += np.float32(400.0)                           # one box leaves the room
    a.update(mats)
    good = info_bounds(a.refresh_info())
    small = good.copy(); small[3] = np.float32(150.0)          # hi.x short of it
    rd = cuda(_rays(40000, seed))
    b.update_device(cuda(mats), bounds=small.reshape(2, 3))
    st = b.device_update_status()
    assert st["bounds_violated"] == 1 and st["rejected_instances"] == 0, st
    occ = b.any_hit(rd); torch.cuda.synchronize()              # too small a pad may cost hits, never the process
    assert occ.shape[0] == 40000
    mats2 = _mats(isd, n_boxes, seed, 2).copy()
    mats2[5, 12] += np.float32(400.0)
    a.update(mats2)
    b.update_device(cuda(mats2), bounds=info_bounds(a.refresh_info()).reshape(2, 3))
    assert b.device_update_status()["bounds_violated"] == 0
    gf = hr.Scene(ctx, isd.flatten(mats2))
    assert_same(answers(b, rd), answers(gf, rd), "correct bounds again: against the flattened scene")
    assert_same(answers(b, rd), answers(a, rd), "correct bounds again: against the host-updated scene")   # whose top level the far box may have re-built
    for g in (a, b, gf):
        g.close()
    g = hr.InstancedScene(ctx, isd, shared=True)
    before = g.read_records()
    for bad in ([0, 0, 0, 1, np.nan, 1], [0, 0, 2, 1, 1, 1]):
        with pytest.raises(hr.HRError) as e:
            g.update_device(cuda(mats2), bounds=np.array(bad, np.float32).reshape(2, 3))
        assert "HR_ERR_INVALID_ARG" in str(e.value)
    gp = hr.InstancedScene(ctx, isd)
    with pytest.raises(hr.HRError) as e:
        gp.update_device(cuda(mats2))
    assert "HR_ERR_INVALID_ARG" in str(e.value) and "shared" in str(e.value)
    assert hr.lib().hr_scene_update_instances_device(g.h, None, None, None) == 1   # HR_ERR_INVALID_ARG: NULL matrices
    assert np.array_equal(g.read_records(), before) and g.device_update_stats()["launches"] == 0, "errors enqueue nothing"
    g.close(); gp.close()


# ---- 6. mirror hand-over -----------------------------------------------------------------------------------------------------------------------
def test_host_calls_after_a_device_update_read_the_matrices_back_once(hr, ctx):
    """device update, host update, device update, rebuild_top_level, update_meshes on the deformable scene of tests/shared_deform_cases.py:
    the flattened scene's answers after every step; one stream wait at each host call that follows a device update, none elsewhere"""
    isd = sc.scene()
    g = hr.InstancedScene(ctx, isd, shared=True, deformable=sc.FLAGS)
    d, _, rays = sc.step_inputs(isd, 0)
    rd = cuda(rays)

    def check(cur, mats, what, waits):
        gf = hr.Scene(ctx, cur.flatten(mats))
        assert_same(answers(g, rd), answers(gf, rd), what)
        gf.close()
        assert g.device_update_stats()["stream_waits"] == waits, (what, g.device_update_stats())

    bounds = np.array([-50, -50, -50, 200, 200, 200], np.float32).reshape(2, 3)   # given: the device updates themselves never wait
    g.update_device(cuda(sc.moved(isd, 1)), bounds=bounds); check(isd, sc.moved(isd, 1), "device update", 0)
    g.update(sc.moved(isd, 2)); check(isd, sc.moved(isd, 2), "host update after a device update", 1)
    g.update(sc.moved(isd, 3)); check(isd, sc.moved(isd, 3), "host update after a host update", 1)
    g.update_device(cuda(sc.moved(isd, 4)), bounds=bounds); check(isd, sc.moved(isd, 4), "device update after host updates", 1)
    before = g.top_level_rebuilds
    g.rebuild_top_level()
    assert g.top_level_rebuilds == before + 1
    check(isd, sc.moved(isd, 4), "re-build after a device update: over the device's matrices", 2)
    g.update_device(cuda(sc.moved(isd, 5)), bounds=bounds); check(isd, sc.moved(isd, 5), "device update on the re-built top level", 2)
    g.update_meshes([entry(d, sc.FIELD, "exact"), entry(d, sc.BOX, "exact")]); check(d, sc.moved(isd, 5), "mesh update after a device update", 3)
    g.update_device(cuda(sc.moved(isd, 6)), bounds=bounds); check(d, sc.moved(isd, 6), "device update over the deformed meshes' bounds", 3)
    g.update_device(cuda(sc.moved(isd, 6)), bounds=bounds); check(d, sc.moved(isd, 6), "the same matrices again", 3)
    twin = hr.InstancedScene(ctx, isd, shared=True, deformable=sc.FLAGS)
    twin.update_meshes([entry(d, sc.FIELD, "exact"), entry(d, sc.BOX, "exact")])
    twin.rebuild_top_level(); twin.update(sc.moved(isd, 6))
    # the twin re-built over other matrices: only the records can be compared, by instance
    ra, rb = g.read_records(), twin.read_records()
    key = lambda r: r[np.argsort(r[:, 140:144].copy().view(np.uint32)[:, 0])]
    assert np.array_equal(key(ra), key(rb)), "records after the hand-overs equal a host-only twin's"
    g.close(); twin.close()


# ---- 7. motion vectors -------------------------------------------------------------------------------------------------------------------------
def test_motion_vectors_follow_a_device_update(hr, ctx):
    n_boxes, seed, W, H = 9, 5, 64, 48
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    a, b = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
    cams = helpers.cameras("cornell", W / H, 3, 1.0)
    light = helpers.light_for("cornell", "soft")
    for f in (1, 2):
        mats = _mats(isd, n_boxes, seed, 3 * f)
        ubo = synth.make_ubo(cams[f], cams[f - 1], light)
        a.motion_begin_frame(); a.update(mats)
        b.motion_begin_frame(); b.update_device(cuda(mats))
        ia, ib = a.gbuffer(ubo, W, H, motion=True), b.gbuffer(ubo, W, H, motion=True)
        for k in ia:
            assert np.array_equal(ia[k].cpu().numpy().view(np.uint8), ib[k].cpu().numpy().view(np.uint8)), f"frame {f}: {k}"
        still = a.gbuffer(ubo, W, H)
        assert not np.array_equal(still["gb2"].cpu().numpy().view(np.uint8), ia["gb2"].cpu().numpy().view(np.uint8)), "the moving half shows in GB2.zw"
    a.close(); b.close()


# ---- 8. passes ---------------------------------------------------------------------------------------------------------------------------------
def test_passes_after_a_device_update(hr, ctx):
    """shadows mask, AO (its entry table follows grid_lo / grid_hi and geometry_epoch), DDGI and reflections at 96x64 on two opted-in twins, one
    updated by the host, one from device memory, over three frames: every image byte-equal"""
    import torch
    n_boxes, seed, W, H = 9, 5, 96, 64
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    a, b = [hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes() for _ in range(2)]
    lo, hi = isd.flatten().bounds()
    rig = Rig(W, H, lo, hi, probes=(3, 3, 3), rays=32)
    pa, pb = Passes(hr, ctx, rig, 1, ground_truth=False), Passes(hr, ctx, rig, 1, ground_truth=False)
    sa, sb = hr.RayTracedShadows(ctx, W, H), hr.RayTracedShadows(ctx, W, H)
    cams = helpers.cameras("cornell", W / H, 4, 1.0)
    light = helpers.light_for("cornell", "soft")
    rng = np.random.RandomState(2)
    prev = None
    for f in range(3):
        mats = _mats(isd, n_boxes, seed, 2 * f)
        a.update(mats)
        b.update_device(cuda(mats), bounds=None if f != 1 else info_bounds(a.refresh_info()).reshape(2, 3))
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f else None, light)
        cur = mirrors(gbuffer_np(b, ubo, W, H))
        cur_a = mirrors(gbuffer_np(a, ubo, W, H))
        for k in cur:
            assert np.array_equal(cur[k], cur_a[k]), f"frame {f}: G-buffer {k}"
        prev = prev if prev is not None else cur
        fi = rig.inputs(hr, helpers.to_cuda(cur), helpers.to_cuda(prev), ubo, f)
        orient = synth_env.random_orientation(rng)
        snap_a, snap_b = pa.render(a, fi, ubo, orient), pb.render(b, fi, ubo, orient)
        assert_equal_snapshots(snap_a, snap_b, f"frame {f}: host-updated against device-updated")
        assert snap_b["ao_rays"] > 0 and snap_b["refl_rays"] > 0
        sa.render(a, fi); sb.render(b, fi)
        torch.cuda.synchronize()
        assert np.array_equal(sa.image(sa.IMG_MASK).cpu().numpy().view(np.uint8), sb.image(sb.IMG_MASK).cpu().numpy().view(np.uint8)), f"frame {f}: shadows mask"
        prev = cur
    for p in (pa, pb, sa, sb, a, b):
        p.close()


# ---- 9. capture --------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_update_reads_the_matrix_buffer_at_replay(hr, ctx):
    """one linear chain on a side stream: update_device(buf, bounds) then any_hit(rays); frame-1 and frame-2 matrices written into buf before a
    replay give the eager answers for those matrices; measuring the bounds under capture is refused and leaves the capture usable"""
    import torch
    n_boxes, seed = 70, 9
    isd = synth.instanced_cornell(n_boxes, seed=seed)
    g, eager = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
    rd = cuda(_rays(40000, seed))
    bounds = np.array([-20, -20, -20, 130, 130, 130], np.float32).reshape(2, 3)
    buf = cuda(_mats(isd, n_boxes, seed, 0))
    g.update_device(buf, bounds=bounds)                       # the first call allocates: eager
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    waits = g.device_update_stats()["stream_waits"]
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(hr.HRError) as e:
            g.update_device(buf, bounds=None)
        assert "HR_ERR_INVALID_ARG" in str(e.value) and "captur" in str(e.value)
        g.update_device(buf, bounds=bounds)
        occ = g.any_hit(rd)
    assert g.device_update_stats()["stream_waits"] == waits
    for f in (1, 2):
        mats = _mats(isd, n_boxes, seed, f)
        buf.copy_(cuda(mats))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager.update_device(cuda(mats), bounds=bounds)
        assert np.array_equal(occ.cpu().numpy(), eager.any_hit(rd).cpu().numpy()), f"replay with frame {f}'s matrices"
        assert np.array_equal(g.read_records(), eager.read_records())
        gf = hr.Scene(ctx, isd.flatten(mats))
        assert np.array_equal(occ.cpu().numpy(), gf.any_hit(rd).cpu().numpy()), f"replay with frame {f}'s matrices against the flattened scene"
        gf.close()
    # the status follows the REPLAYS: once an update has been captured every status call reads the device's block back
    st2 = g.device_update_status()
    assert st2["rejected_instances"] == 0 and st2["bounds_violated"] == 0, st2
    bad = _mats(isd, n_boxes, seed, 3).copy()
    bad[4, 5] = np.nan
    buf.copy_(cuda(bad))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    st3 = g.device_update_status()
    assert st3["rejected_instances"] == 1 and st3["top_cost_ratio"] != st2["top_cost_ratio"], (st2, st3)
    # host calls between replays: each reads the matrices back, so the second update(X) is not mistaken for "nothing changed"
    X = _mats(isd, n_boxes, seed, 5)
    gx = hr.Scene(ctx, isd.flatten(X))
    want_x = gx.any_hit(rd).cpu().numpy()
    gx.close()
    before = g.device_update_stats()["stream_waits"]
    g.update(X)
    assert np.array_equal(g.any_hit(rd).cpu().numpy(), want_x), "host update after a replay"
    m6 = _mats(isd, n_boxes, seed, 6)
    buf.copy_(cuda(m6))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    g6 = hr.Scene(ctx, isd.flatten(m6))
    assert np.array_equal(occ.cpu().numpy(), g6.any_hit(rd).cpu().numpy()), "replay after a host update"
    g6.close()
    g.update(X)
    assert np.array_equal(g.any_hit(rd).cpu().numpy(), want_x), "the same host matrices again after another replay: the scene must follow"
    assert g.device_update_stats()["stream_waits"] == before + 2, "one read-back per host call on a scene whose update was captured"
    del graph
    g.close(); eager.close()


# ---- 10. launch count --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boxes", [0, 5, 70, 600])
def test_two_launches_per_update_of_a_small_scene(hr, ctx, n_boxes):
    isd = synth.instanced_cornell(n_boxes, seed=3)
    g = hr.InstancedScene(ctx, isd, shared=True)
    assert g.device_update_stats() == dict(launches=0, stream_waits=0)
    bounds = np.array([-20, -20, -20, 130, 130, 130], np.float32).reshape(2, 3)
    for k, f in enumerate((1, 2, 2)):
        g.update_device(cuda(_mats(isd, n_boxes, 3, f)), bounds=bounds if k else None)
        assert g.device_update_stats() == dict(launches=LAUNCHES_SMALL * (k + 1), stream_waits=1)
    gf = hr.Scene(ctx, isd.flatten(_mats(isd, n_boxes, 3, 2)))
    rd = cuda(_rays(5000, 3))
    assert_same(answers(g, rd), answers(gf, rd), "after the updates")
    g.close(); gf.close()
