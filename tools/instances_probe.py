"""GPU developer tool: what hr_scene_update_instances costs and what the refitted tree costs the trace kernels.
Scene: the bench building (sponza_like(detail), identity instance) + `--movers` instances of a cube / pyramid mesh flying through it.
  * update: wall clock of N back-to-back updates (matrix upload + vertex transform + reference gather + per-level refit), per update;
  * quality: the shadows trace stage on the instanced scene after `--frames` updates of motion against hr_scene_create over the same world
    vertices (a fresh SAH build), same G-buffer — masks must be equal, the time ratio is the price of never rebuilding.
    python tools/instances_probe.py [--detail 1.0 --movers 200 --frames 30 --width 1920 --height 1080]
--deform: what hr_scene_update_meshes costs.  Scene: the building + `--meshes` deforming heightfields (`--field` cells a side) placed `--copies`
times each, created by hr_scene_create_instanced_shared_deformable.  Reported, per frame of a wave: all meshes in ONE call against one call each
(bounds given, so nothing waits; and measured, with the wait); the same triangle count through hr_scene_update_vertices on a flat deformable
scene; re-creating the shared scene (the only route before this call existed); the shadows trace stage on the refitted scene against one
created fresh over the same deformed meshes (masks must be equal).
--shared --passes: the ray_trace stage of AO (4 spp), DDGI (16x8x16 probes, 256 rays) and reflections (half resolution) on the shared scene, opted
in to the two-level passes, next to the PRIVATE-COPY scene of the same desc and matrices (the single-level kernels: the yardstick).  Both scenes
see the same G-buffer; they are timed in alternating rounds of 10 profiled frames after a warm-up and the per-round averages are printed as
mean [min, max]; masks, radiance and trace images must be equal.
--shared --device: what hr_scene_update_instances_device costs next to hr_scene_update_instances on twin shared scenes over the same matrices
(already resident on the GPU for the device path).  Every frame is timed on its own (update, then wait for the stream) and the MEDIAN over the
frames is reported: the host path twice (`host_ms`, `host_ms_again`: their difference is the run-to-run spread), the device path with the bounds
given and with the bounds measured; then the same frames back to back without waiting in between (what the calling thread pays per frame).
Any-hit answers of 20 000 rays must agree after the last frame.  --host-only: the host path's numbers alone (a library built from a revision
that does not have the device path, selected with HR_LIBRARY).
--shared --deform --device-rebuild: the --deform probe, then hr_scene_rebuild_meshes_device over every deforming mesh (csrc/deform_redeal.hip): event
time of the call, the shadow trace on the re-dealt trees beside the refitted and the fresh ones, and per mesh the cost ratio refitted / re-dealt.
--shared --device-rebuild: what hr_scene_rebuild_top_level_device costs.  Per size of synth.instanced_cornell (70, 600, 3300, 4096 boxes: the
last one instance above the one-workgroup sort's limit), medians over `--reps` calls timed one by one (call, then wait for the stream) after a
warm-up: the device re-build; hr_scene_rebuild_top_level on a twin that has just taken a device update (so its wall time includes the read-back
it needs); a device update with the threshold off and with a threshold that never fires (what the predicated launches add to a frame on which
nothing is re-built), one by one and back to back.  Then, on the scene of main() after `--frames` frames of motion through device updates: the
shadows trace stage on the device-built top level against a fresh host SAH top level over the same matrices (masks must be equal), and the
ratio of their half-area sums (numpy, over the nodes and records read back: top_area_np below).
--shared --hidden FRACTION: after the figures above, that share of the movers is hidden by instance mask (hr_scene_set_instance_masks: mask 0,
a seeded random subset) and the shadows trace stage is timed again on the same G-buffer: `shadow_trace_ms_hidden` next to
`shadow_trace_ms_refitted` is what despawning by mask buys; the mask image must equal the one of a shared scene created from the visible
subset."""
import argparse, json, math, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--movers", type=int, default=200)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--shared", action="store_true", help="hr_scene_create_instanced_shared: one BVH per mesh, two-level walk")
    ap.add_argument("--deform", action="store_true", help="hr_scene_update_meshes on a shared scene with deforming meshes")
    ap.add_argument("--passes", action="store_true", help="with --shared: AO / DDGI / reflections trace stages, shared against private copies")
    ap.add_argument("--device", action="store_true", help="with --shared: hr_scene_update_instances_device against the host update, per frame")
    ap.add_argument("--device-rebuild", action="store_true", help="with --shared: hr_scene_rebuild_top_level_device against the host re-build, and the trace on either tree")
    ap.add_argument("--hidden", type=float, default=0.0, help="with --shared: hide this share of the movers by instance mask and time the shadow trace again")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-only", action="store_true", help="with --shared --device: time the host path alone")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--field", type=int, default=48)
    a = ap.parse_args()
    if a.deform:
        return deform_probe(a)
    if a.device_rebuild:
        assert a.shared, "--device-rebuild times the device re-build of a shared scene's top level: give --shared"
        return rebuild_probe(a)
    if a.device:
        assert a.shared, "--device times the device-side update of a shared scene: give --shared"
        return device_probe(a)
    if a.passes:
        assert a.shared, "--passes compares a shared scene with its private-copy twin: give --shared"
        return passes_probe(a)
    import torch
    from hybrid_rendering_amd import api as hr, synth
    W, H = a.width, a.height
    building = synth.sponza_like(a.detail)
    small = synth.instanced_cornell(2)
    cube, pyr = small.meshes[1], small.meshes[2]
    lo, hi = building.bounds()
    rng = np.random.RandomState(1)
    base = [(rng.uniform(lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo)), rng.uniform(-1, 1, 3), rng.uniform(0, 6.28), rng.uniform(6, 30, 3), rng.uniform(-2, 2, 3)) for _ in range(a.movers)]

    def instances(f):
        out = [(synth.model_matrix(), 0, 1)]
        for i, (p, ax, ang, sc, vel) in enumerate(base):
            out.append((synth.model_matrix(p + vel * f, ax, ang + 0.05 * f, sc), 1 + (i & 1), 2 + i))
        return out
    isd = synth.InstancedSceneData(meshes=[building, cube, pyr], instances=instances(0), materials=building.materials)
    ctx = hr.Context(0)
    t0 = time.perf_counter()
    g = hr.InstancedScene(ctx, isd, shared=True) if a.shared else hr.InstancedScene(ctx, isd)
    t_create = time.perf_counter() - t0
    mats = [synth.InstancedSceneData(isd.meshes, instances(f), isd.materials).matrices() for f in range(a.frames + 1)]
    for m in mats[:3]:
        g.update(m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for m in mats:
        g.update(m)
    torch.cuda.synchronize()
    upd_ms = (time.perf_counter() - t0) / len(mats) * 1e3
    info = g.refresh_info()
    res = dict(tris=info.n_tris, nodes=info.n_nodes, depth=info.max_depth, instances=a.movers + 1, create_s=round(t_create, 2), update_ms=round(upd_ms, 4),
               top_level_rebuilds=g.top_level_rebuilds, auto_rebuild=os.environ.get("HR_TOP_LEVEL_REBUILD", "1"))
    # quality of the refitted tree after `frames` updates
    light = synth.sponza_light()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(2)]
    ubo = synth.make_ubo(cams[1], cams[0], light)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    flat = hr.Scene(ctx, isd.flatten(mats[-1]))
    gb = flat.gbuffer(ubo, W, H)
    fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d)
    out = {}
    runs = [("refitted", g), ("rebuilt", flat)]
    if a.hidden > 0.0:
        assert a.shared, "--hidden hides instances of a shared scene by mask: give --shared"
        gone = np.sort(1 + np.random.RandomState(7).permutation(a.movers)[:int(round(a.hidden * a.movers))])
        keep = [i for i in range(a.movers + 1) if i not in set(gone.tolist())]
        last = instances(a.frames)
        runs += [("hidden", g), ("subset", hr.InstancedScene(ctx, synth.InstancedSceneData(isd.meshes, [last[i] for i in keep], isd.materials), shared=True))]
    for tag, sc in runs:
        if tag == "hidden":   # behind the timing of the unmasked scene
            masks = np.full(a.movers + 1, 0xFF, np.uint8)
            masks[gone] = 0
            g.set_instance_masks(masks)
        p = hr.RayTracedShadows(ctx, W, H)
        p.params.exact = 0
        for k in range(6):
            fi.num_frames = k
            p.render(sc, fi)
        p.set_profiling(True)
        acc = {}
        for k in range(6, 26):
            fi.num_frames = k
            p.render(sc, fi)
            for n, t, b in p.stage_times():
                acc[n] = acc.get(n, 0.0) + t / 20
        torch.cuda.synchronize()
        out[tag] = (p.image(p.IMG_MASK).cpu().numpy().copy(), acc)
        p.close()
    assert np.array_equal(out["refitted"][0], out["rebuilt"][0]), "masks differ between the refitted and the rebuilt tree"
    res["shadow_trace_ms_refitted"] = round(out["refitted"][1]["ray_trace"], 4)
    res["shadow_trace_ms_rebuilt"] = round(out["rebuilt"][1]["ray_trace"], 4)
    res["masks_equal"] = True
    if a.hidden > 0.0:
        assert np.array_equal(out["hidden"][0], out["subset"][0]), "masks differ between the masked scene and the scene created from the visible subset"
        res["hidden_instances"] = int(len(gone))
        res["shadow_trace_ms_hidden"] = round(out["hidden"][1]["ray_trace"], 4)
        res["shadow_trace_ms_subset"] = round(out["subset"][1]["ray_trace"], 4)
    if a.shared:
        res["kind"] = "shared"
    print(json.dumps(res))


def device_probe(a):
    import torch
    from hybrid_rendering_amd import api as hr, synth
    building = synth.sponza_like(a.detail)
    small = synth.instanced_cornell(2)
    cube, pyr = small.meshes[1], small.meshes[2]
    lo, hi = building.bounds()
    rng = np.random.RandomState(1)   # the scene and the motion of main()
    base = [(rng.uniform(lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo)), rng.uniform(-1, 1, 3), rng.uniform(0, 6.28), rng.uniform(6, 30, 3), rng.uniform(-2, 2, 3)) for _ in range(a.movers)]

    def instances(f):
        return [(synth.model_matrix(), 0, 1)] + [(synth.model_matrix(p + vel * f, ax, ang + 0.05 * f, sc), 1 + (i & 1), 2 + i) for i, (p, ax, ang, sc, vel) in enumerate(base)]
    isd = synth.InstancedSceneData(meshes=[building, cube, pyr], instances=instances(0), materials=building.materials)
    ctx = hr.Context(0)
    mats = [synth.InstancedSceneData(isd.meshes, instances(f), isd.materials).matrices() for f in range(a.frames + 1)]
    g_host = hr.InstancedScene(ctx, isd, shared=True)

    def per_frame(fn, frames):
        """(median of the frames timed one by one, mean of the frames enqueued back to back), ms"""
        for m in frames[:3]:
            fn(m)
        torch.cuda.synchronize()
        one = []
        for m in frames:
            t0 = time.perf_counter()
            fn(m)
            torch.cuda.synchronize()
            one.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for m in frames:
            fn(m)
        torch.cuda.synchronize()
        return round(float(np.median(one)), 4), round((time.perf_counter() - t0) / len(frames) * 1e3, 4)
    res = dict(kind="shared, device-side instance update", instances=a.movers + 1, frames=len(mats))
    res["host_ms"], res["host_ms_back_to_back"] = per_frame(g_host.update, mats)
    if not a.host_only:
        g_dev = hr.InstancedScene(ctx, isd, shared=True)
        box = np.array([np.inf] * 3 + [-np.inf] * 3)
        for m in mats:   # bounds that hold for every frame: the union of the host path's conservative ones
            g_host.update(m)
            i = g_host.refresh_info()
            box = np.concatenate([np.minimum(box[:3], list(i.bounds_lo)), np.maximum(box[3:], list(i.bounds_hi))])
        bounds = box.astype(np.float32).reshape(2, 3)
        dev = [torch.from_numpy(m).cuda() for m in mats]
        res["device_ms_bounds_given"], res["device_ms_bounds_given_back_to_back"] = per_frame(lambda m: g_dev.update_device(m, bounds=bounds), dev)
        res["device_ms_bounds_measured"], res["device_ms_bounds_measured_back_to_back"] = per_frame(lambda m: g_dev.update_device(m), dev)
        res["device_status"], res["device_stats"] = g_dev.device_update_status(), g_dev.device_update_stats()
    res["host_ms_again"], res["host_ms_again_back_to_back"] = per_frame(g_host.update, mats)
    res["host_spread_ms"] = round(abs(res["host_ms"] - res["host_ms_again"]), 4)
    res["host_top_level_rebuilds"] = g_host.top_level_rebuilds
    if not a.host_only:
        r = np.zeros((20000, 8), np.float32)
        r[:, :3] = rng.uniform(lo, hi, (20000, 3))
        d = rng.normal(size=(20000, 3))
        r[:, 4:7], r[:, 3], r[:, 7] = d / np.linalg.norm(d, axis=1, keepdims=True), 1e4, 0.01
        rd = torch.from_numpy(r).cuda()
        assert np.array_equal(g_host.any_hit(rd).cpu().numpy(), g_dev.any_hit(rd).cpu().numpy()), "any-hit answers differ between the host- and the device-updated scene"
        res["answers_equal"] = True
    print(json.dumps(res))


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
        out[i, :3] = np.where(lo32.astype(np.float64) > l, np.nextafter(lo32, np.float32(-np.inf)), lo32)
        out[i, 3:] = np.where(hi32.astype(np.float64) < h, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return out


def top_area_np(isd, mats, nodes, records, pad):
    """sum over a shared scene's top-level nodes of the half area of the box of their children (leaves: instance box -+ pad in fp32); the
    topology from the nodes (csrc/bvh.h Node8: counts, child_base, tri_base), the leaves' instances from the records (byte 140)"""
    boxes, pad = instance_boxes_np(isd, mats), np.float32(pad)
    inst_of_leaf = records[:, 140:144].copy().view(np.uint32)[:, 0]
    kids, order, at = {}, [0], 0
    while at < len(order):
        n = nodes[order[at]]
        n_int, nc = int(n[15]) & 15, int(n[15]) >> 4
        child_base, leaf_base = int(n[16:20].copy().view(np.uint32)[0]), int(n[20:24].copy().view(np.uint32)[0])
        kids[order[at]] = ([child_base + c for c in range(n_int)], [leaf_base + j for j in range(nc - n_int)])
        order += kids[order[at]][0]
        at += 1
    box, total = {}, 0.0
    for slot in reversed(order):
        lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for c in kids[slot][0]:
            lo, hi = np.minimum(lo, box[c][0]), np.maximum(hi, box[c][1])
        for l in kids[slot][1]:
            lo, hi = np.minimum(lo, boxes[inst_of_leaf[l]][:3] - pad), np.maximum(hi, boxes[inst_of_leaf[l]][3:] + pad)
        box[slot] = (lo, hi)
        d = hi.astype(np.float64) - lo.astype(np.float64)
        total += d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    return total, len(order)


def rebuild_probe(a):
    import torch
    from hybrid_rendering_amd import api as hr, synth
    _mats = lambda isd, n_boxes, seed, frame: synth.InstancedSceneData(isd.meshes, synth.instanced_cornell_instances(n_boxes, seed=seed, frame=frame), isd.materials).matrices()
    ctx = hr.Context(0)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()

    def one_by_one(fn, reps, before=None):
        out = []
        for k in range(reps + 5):   # 5 warm-up calls
            if before:
                before(k)
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(out[5:])), 4)

    def back_to_back(fn, reps):
        for k in range(5):
            fn(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(reps):
            fn(k)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / reps * 1e3, 4)
    res = dict(kind="shared, device re-build of the top level", reps=a.reps, sizes={})
    bounds = np.array([-20, -20, -20, 130, 130, 130], np.float32).reshape(2, 3)
    for n_boxes in (70, 600, 3300, 4096):
        isd = synth.instanced_cornell(n_boxes, seed=4)
        dev = [cuda(_mats(isd, n_boxes, 4, f)) for f in (88, 89, 90, 91)]
        g, twin = hr.InstancedScene(ctx, isd, shared=True), hr.InstancedScene(ctx, isd, shared=True)
        g.update_device(dev[0], bounds=bounds)
        r = dict(top_level_nodes=len(hr.shared_top_fixed_shape(n_boxes + 1)[0]))
        r["device_rebuild_ms"] = one_by_one(lambda k: g.rebuild_top_level_device(), a.reps, before=lambda k: g.update_device(dev[k & 3], bounds=bounds))
        r["host_rebuild_after_device_update_ms"] = one_by_one(lambda k: twin.rebuild_top_level(), max(10, a.reps // 5), before=lambda k: twin.update_device(dev[k & 3], bounds=bounds))
        g.set_device_rebuild_threshold(0.0)
        r["update_ms_threshold_off"] = one_by_one(lambda k: g.update_device(dev[k & 3], bounds=bounds), a.reps)
        r["update_ms_threshold_off_back_to_back"] = back_to_back(lambda k: g.update_device(dev[k & 3], bounds=bounds), a.reps)
        launches = g.device_update_stats()["launches"]
        g.set_device_rebuild_threshold(1e6)
        before = g.device_rebuild_status()["rebuilds_done"]
        r["update_ms_threshold_never_fires"] = one_by_one(lambda k: g.update_device(dev[k & 3], bounds=bounds), a.reps)
        r["update_ms_threshold_never_fires_back_to_back"] = back_to_back(lambda k: g.update_device(dev[k & 3], bounds=bounds), a.reps)
        assert g.device_rebuild_status()["rebuilds_done"] == before
        r["update_ms_off_again"] = (g.set_device_rebuild_threshold(0.0), one_by_one(lambda k: g.update_device(dev[k & 3], bounds=bounds), a.reps))[1]
        res["sizes"][n_boxes + 1] = r
        g.close(); twin.close()
    # the trace on either tree
    W, H = a.width, a.height
    building = synth.sponza_like(a.detail)
    small = synth.instanced_cornell(2)
    cube, pyr = small.meshes[1], small.meshes[2]
    lo, hi = building.bounds()
    rng = np.random.RandomState(1)   # the scene and the motion of main()
    base = [(rng.uniform(lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo)), rng.uniform(-1, 1, 3), rng.uniform(0, 6.28), rng.uniform(6, 30, 3), rng.uniform(-2, 2, 3)) for _ in range(a.movers)]
    inst = lambda f: [(synth.model_matrix(), 0, 1)] + [(synth.model_matrix(p + vel * f, ax, ang + 0.05 * f, sc), 1 + (i & 1), 2 + i) for i, (p, ax, ang, sc, vel) in enumerate(base)]
    isd = synth.InstancedSceneData(meshes=[building, cube, pyr], instances=inst(0), materials=building.materials)
    mats = synth.InstancedSceneData(isd.meshes, inst(a.frames), isd.materials).matrices()
    scenes = dict(stale=hr.InstancedScene(ctx, isd, shared=True), device_built=hr.InstancedScene(ctx, isd, shared=True), host_sah=hr.InstancedScene(ctx, isd, shared=True))
    for sc_ in scenes.values():
        sc_.update_device(cuda(mats))
    scenes["device_built"].rebuild_top_level_device()
    scenes["host_sah"].rebuild_top_level()
    top = a.movers + 1
    area = {tag: top_area_np(isd, mats, sc_.read_bvh()[0][:top], sc_.read_records(), sc_.refresh_info().box_pad)[0] for tag, sc_ in scenes.items()}
    light = synth.sponza_light()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(2)]
    ubo = synth.make_ubo(cams[1], cams[0], light)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    gb = scenes["host_sah"].gbuffer(ubo, W, H)
    fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d)
    passes = {tag: hr.RayTracedShadows(ctx, W, H) for tag in scenes}
    for p in passes.values():
        p.params.exact = 0
    for tag, p in passes.items():
        for k in range(6):
            fi.num_frames = k
            p.render(scenes[tag], fi)
    torch.cuda.synchronize()
    rounds = {tag: [] for tag in scenes}
    for r_ in range(a.rounds):   # alternating rounds of 10 profiled frames: every tree sees the same neighbours on the machine
        for tag, p in passes.items():
            p.set_profiling(True)
            p.stage_times()
            for k in range(6 + 10 * r_, 16 + 10 * r_):
                fi.num_frames = k
                p.render(scenes[tag], fi)
            torch.cuda.synchronize()
            rounds[tag].append(dict((s_, ms) for s_, ms, _ in p.stage_times())["ray_trace"])
            p.set_profiling(False)
    masks = {tag: p.image(p.IMG_MASK).cpu().numpy().copy() for tag, p in passes.items()}
    assert all(np.array_equal(m, masks["host_sah"]) for m in masks.values()), "masks differ between the top levels"
    res["trace"] = dict(width=W, height=H, instances=top, frames_of_motion=a.frames, masks_equal=True, rounds=a.rounds,
                        half_area_sum={k: round(v, 1) for k, v in area.items()},
                        half_area_device_built_over_host_sah=round(area["device_built"] / area["host_sah"], 4), half_area_stale_over_host_sah=round(area["stale"] / area["host_sah"], 4))
    for tag, v in rounds.items():
        res["trace"][f"shadow_trace_ms_{tag}"] = [round(float(np.mean(v)), 4), round(min(v), 4), round(max(v), 4)]
    print(json.dumps(res))


def passes_probe(a):
    import torch
    from hybrid_rendering_amd import api as hr, api_gi, api_reflections, synth, synth_env
    W, H = a.width, a.height
    building = synth.sponza_like(a.detail)
    small = synth.instanced_cornell(2)
    cube, pyr = small.meshes[1], small.meshes[2]
    lo, hi = building.bounds()
    rng = np.random.RandomState(1)
    inst = [(synth.model_matrix(), 0, 1)]
    for i in range(a.movers):   # the default scene of main() after `frames` frames of motion
        p, ax, ang, sc, vel = rng.uniform(lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo)), rng.uniform(-1, 1, 3), rng.uniform(0, 6.28), rng.uniform(6, 30, 3), rng.uniform(-2, 2, 3)
        inst.append((synth.model_matrix(p + vel * a.frames, ax, ang + 0.05 * a.frames, sc), 1 + (i & 1), 2 + i))
    isd = synth.InstancedSceneData(meshes=[building, cube, pyr], instances=inst, materials=building.materials)
    ctx = hr.Context(0)
    scenes = dict(shared=hr.InstancedScene(ctx, isd, shared=True).enable_two_level_passes(), private=hr.InstancedScene(ctx, isd))
    light = synth.sponza_light()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(2)]
    ubo = synth.make_ubo(cams[1], cams[0], light)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    gb = scenes["private"].gbuffer(ubo, W, H)
    low = hr.gbuffer_mip(gb, 1)
    fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d, z_buffer_params=synth.z_buffer_params())
    fl = hr.frame_inputs(low, low, ubo, 0, 0, sob_d, sr_d, cur_full=gb, z_buffer_params=synth.z_buffer_params())
    ddgi_u = synth_env.ddgi_uniforms(lo, hi, probe_counts=(16, 8, 16), rays_per_probe=256, normal_bias=0.1)
    sky = synth_env.sky_cubemap(32)
    f16 = lambda x: torch.from_numpy(x).cuda().view(torch.float16)
    env = api_gi.environment(f16(sky), f16(synth_env.prefiltered_chain(sky, 5)), 32, 5, f16(synth_env.brdf_lut(32)))
    orient = synth_env.random_orientation(np.random.RandomState(1))
    passes = {}
    for tag in scenes:
        ao, gi, rf = hr.RayTracedAO(ctx, W, H, 0), api_gi.DDGI(ctx, W, H, ddgi_u), api_reflections.RayTracedReflections(ctx, W, H, 1)
        ao.params.spp = 4
        for p in (ao, gi, rf):
            p.params.exact = 0
        passes[tag] = dict(ao=ao, ddgi=gi, reflections=rf)

    def frame(tag, k):
        sc, ps = scenes[tag], passes[tag]
        fi.num_frames = fl.num_frames = k
        ps["ao"].render(sc, fi); ps["ddgi"].render(sc, fi, env, orient); ps["reflections"].render(sc, fl, env, ps["ddgi"])
    for tag in scenes:
        for k in range(6):
            frame(tag, k)
    torch.cuda.synchronize()
    rounds = {tag: {n: [] for n in ("ao", "ddgi", "reflections")} for tag in scenes}
    for r in range(a.rounds):
        for tag in scenes:   # alternating: both kinds see the same neighbours on the machine
            for p in passes[tag].values():
                p.set_profiling(True)
                p.stage_times()
            for k in range(6 + 10 * r, 16 + 10 * r):
                frame(tag, k)
            torch.cuda.synchronize()
            for n, p in passes[tag].items():
                rounds[tag][n].append(dict((s_, ms) for s_, ms, _ in p.stage_times())["ray_trace"])
                p.set_profiling(False)
    img = {tag: (ps["ao"].image(0).cpu().numpy().copy(), ps["ddgi"].image(0).cpu().numpy().copy(), ps["reflections"].image(0).cpu().numpy().copy()) for tag, ps in passes.items()}
    for x, y, what in zip(img["shared"], img["private"], ("AO masks", "DDGI radiance", "reflections trace image")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), what + " differ between the shared and the private-copy scene"
    res = dict(kind="shared against private copies, trace stages", width=W, height=H, instances=a.movers + 1, tris=scenes["private"].refresh_info().n_tris, rounds=a.rounds, images_equal=True)
    for tag in scenes:
        info = scenes[tag].refresh_info()
        res[tag + "_scene_bytes"] = int(info.node_bytes) + int(info.tri_bytes)
        for n, v in rounds[tag].items():
            res[f"{n}_trace_ms_{tag}"] = [round(float(np.mean(v)), 4), round(min(v), 4), round(max(v), 4)]
    print(json.dumps(res))


def deform_probe(a):
    import torch
    from hybrid_rendering_amd import api as hr, synth
    W, H = a.width, a.height
    building = synth.sponza_like(a.detail)
    lo, hi = building.bounds()
    rng = np.random.RandomState(2)
    N = a.meshes
    fields = [synth.heightfield(a.field, size=60.0, height=10.0, seed=11 + k) for k in range(N)]
    fields = [synth.SceneData(f.verts, f.normals, f.tri_material, f.tri_mesh_id, building.materials, f.name) for f in fields]
    inst = [(synth.model_matrix(), 0, 1)]
    for k in range(N):
        for c in range(a.copies):
            at = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo))
            inst.append((synth.model_matrix(at, (0, 1, 0), rng.uniform(0, 6.28), rng.uniform(0.5, 1.5, 3)), 1 + k, 2 + len(inst)))
    isd = synth.InstancedSceneData(meshes=[building] + fields, instances=inst, materials=building.materials)
    flags = [0] + [1] * N
    ctx = hr.Context(0)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    t0 = time.perf_counter()
    g = hr.InstancedScene(ctx, isd, shared=True, deformable=flags)
    t_create = time.perf_counter() - t0
    frames = [synth.deform_meshes(isd, f, "wave", range(1, N + 1)) for f in range(1, 4)]
    dev = [[dict(mesh_idx=k, positions=cuda(d.meshes[k].verts), normals=cuda(d.meshes[k].normals), bounds=d.meshes[k].bounds()) for k in range(1, N + 1)] for d in frames]
    measured = [[{k: v for k, v in u.items() if k != "bounds"} for u in ups] for ups in dev]

    def timed(fn, reps=20):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(i)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / reps * 1e3, 4)
    res = dict(kind="shared, deforming meshes", meshes=N, copies=a.copies, tris_per_mesh=fields[0].n_tris, instances=len(inst), create_s=round(t_create, 2))
    res["update_ms_one_call_bounds_given"] = timed(lambda i: g.update_meshes(dev[i % 3]))
    res["update_ms_one_call_each_bounds_given"] = timed(lambda i: [g.update_meshes([u]) for u in dev[i % 3]])
    res["update_ms_one_call_bounds_measured"] = timed(lambda i: g.update_meshes(measured[i % 3]))
    res["update_ms_one_call_each_bounds_measured"] = timed(lambda i: [g.update_meshes([u]) for u in measured[i % 3]])
    res["stats"] = g.update_meshes_stats()
    res["refit_cost_mesh_1"] = round(g.mesh_refit_cost(1), 4)
    # the same triangles as ONE flat deformable scene (object space, side by side: only the triangle count matters)
    flat_sd = synth.InstancedSceneData(meshes=fields, instances=[(synth.model_matrix((70.0 * k, 0, 0)), k, k) for k in range(N)], materials=building.materials).flatten()
    gd = hr.Scene(ctx, flat_sd, deformable=True)
    pos = [cuda(synth.deform(flat_sd, f, "wave").verts) for f in range(1, 4)]
    res["update_vertices_ms_flat_scene_same_triangles"] = timed(lambda i: gd.update_vertices(pos[i % 3]))
    gd.close()

    def recreate(i):
        s = hr.InstancedScene(ctx, frames[i % 3], shared=True)
        s.close()
    res["recreate_shared_scene_ms"] = timed(recreate, reps=3)
    # the trace on the refitted scene against a scene created fresh over the same meshes
    g.update_meshes(dev[2])
    fresh = hr.InstancedScene(ctx, frames[2], shared=True)
    light = synth.sponza_light()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(2)]
    ubo = synth.make_ubo(cams[1], cams[0], light)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    gb = fresh.gbuffer(ubo, W, H)
    fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d)
    out = {}
    def trace(sc):
        p = hr.RayTracedShadows(ctx, W, H)
        p.params.exact = 0
        for k in range(6):
            fi.num_frames = k
            p.render(sc, fi)
        p.set_profiling(True)
        acc = {}
        for k in range(6, 26):
            fi.num_frames = k
            p.render(sc, fi)
            for n, t, b in p.stage_times():
                acc[n] = acc.get(n, 0.0) + t / 20
        torch.cuda.synchronize()
        r = (p.image(p.IMG_MASK).cpu().numpy().copy(), acc)
        p.close()
        return r
    out["refitted"], out["fresh"] = trace(g), trace(fresh)
    if a.device_rebuild:
        # hr_scene_rebuild_meshes_device over every deforming mesh: event time of the call (the first call allocates and is not timed), the trace
        # on the re-dealt trees, and per mesh the cost ratio refitted / re-dealt (a fresh scene's is 1.0: the host build is the baseline)
        all_meshes = list(range(1, N + 1))
        refitted = [g.mesh_refit_cost(k) for k in all_meshes]
        for _ in range(3):
            g.rebuild_meshes_device(all_meshes)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            g.rebuild_meshes_device(all_meshes)
        e1.record()
        torch.cuda.synchronize()
        res["rebuild_meshes_device_ms"] = round(e0.elapsed_time(e1) / 20, 4)
        res["rebuild_meshes_device_launches_per_call"] = g.device_rebuild_counts()["launches_enqueued"] // 23
        out["redealt"] = trace(g)
        assert np.array_equal(out["redealt"][0], out["fresh"][0]), "masks differ between the re-dealt and the freshly created scene"
        res["shadow_trace_ms_redealt"] = round(out["redealt"][1]["ray_trace"], 4)
        res["refit_cost_per_mesh"] = [dict(mesh=k, refitted=round(r, 4), redealt=round(g.mesh_refit_cost(k), 4), host_built=1.0) for k, r in zip(all_meshes, refitted)]
    assert np.array_equal(out["refitted"][0], out["fresh"][0]), "masks differ between the refitted and the freshly created scene"
    res["shadow_trace_ms_refitted"] = round(out["refitted"][1]["ray_trace"], 4)
    res["shadow_trace_ms_fresh"] = round(out["fresh"][1]["ray_trace"], 4)
    res["masks_equal"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
