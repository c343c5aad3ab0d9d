"""GPU developer tool: what a deformable scene costs (docs/EXPERIMENTS.md "Deformable scenes").
  * update: hr_scene_update_vertices per frame as event time on the stream, a full update and a 10 % range;
  * quality: the shadows trace stage after every few frames of "wave" on the refitted tree, on the same scene after hr_scene_rebuild, and on the
    plain split tree hr_scene_create builds over the same vertices (what giving up spatial splits costs) — masks must be equal — with
    hr_scene_refit_cost beside each, so that the ratio at which refitted / rebuilt crosses 1.25 can be read off;
  * rebuild: wall time of hr_scene_rebuild.
  * --device-rebuild: hr_scene_rebuild_device (csrc/deform_redeal.hip) after the last frame — event time of the call on the stream, the shadows
    trace on the refitted, the re-dealt and the host-rebuilt tree (masks must be equal), the three cost ratios, and what Morton order costs a
    tree that had not decayed (a twin re-dealt at its creation vertices).
    python tools/deform_probe.py [--detail 1.0 --tier standard --frames 30 --every 10 --kind wave --width 1920 --height 1080 --device-rebuild]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--tier", default="standard")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--kind", default="wave")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--device-rebuild", action="store_true", help="hr_scene_rebuild_device after the last frame: its device time, the trace on the refitted / re-dealt / host-rebuilt tree, the cost ratios")
    a = ap.parse_args()
    import torch
    from hybrid_rendering_amd import api as hr, synth
    W, H = a.width, a.height
    sd0 = synth.sponza_like(a.detail, tier=a.tier)
    ctx = hr.Context(0)
    t0 = time.perf_counter()
    g = hr.Scene(ctx, sd0, deformable=True)
    res = dict(tris=sd0.n_tris, nodes=g.info.n_nodes, depth=g.info.max_depth, create_s=round(time.perf_counter() - t0, 2), kind=a.kind)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()

    def timed_updates(sd, first, count, reps=20):
        p, n = cuda(sd.verts[first:first + count]), cuda(sd.normals[first:first + count])
        for _ in range(3):
            g.update_vertices(p, n, first_tri=first)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.update_vertices(p, n, first_tri=first)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    res["update_full_ms"] = round(timed_updates(sd0, 0, sd0.n_tris), 4)
    res["update_tenth_ms"] = round(timed_updates(sd0, sd0.n_tris // 3, sd0.n_tris // 10), 4)

    light = synth.sponza_light()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(2)]
    ubo = synth.make_ubo(cams[1], cams[0], light)
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()

    def trace_ms(scene, fi):
        p = hr.RayTracedShadows(ctx, W, H)
        p.params.exact = 0
        for k in range(6):
            fi.num_frames = k
            p.render(scene, fi)
        p.set_profiling(True)
        acc = 0.0
        for k in range(6, 26):
            fi.num_frames = k
            p.render(scene, fi)
            acc += dict((n, t) for n, t, b in p.stage_times())["ray_trace"] / 20
        torch.cuda.synchronize()
        mask = p.image(p.IMG_MASK).cpu().numpy().copy()
        p.close()
        return acc, mask
    rows = []
    for f in range(a.every, a.frames + 1, a.every):
        sd = synth.deform(sd0, f, a.kind)
        g.update_vertices(cuda(sd.verts), cuda(sd.normals))
        plain = hr.Scene(ctx, sd)
        gb = plain.gbuffer(ubo, W, H)
        fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d)
        cost = g.refit_cost()
        t_refit, m_refit = trace_ms(g, fi)
        fresh = hr.Scene(ctx, sd, deformable=True)   # what hr_scene_rebuild would give, without disturbing the sequence of refits
        t_rebuilt, m_rebuilt = trace_ms(fresh, fi)
        t_plain, m_plain = trace_ms(plain, fi)
        assert np.array_equal(m_refit, m_rebuilt) and np.array_equal(m_refit, m_plain), "masks differ between the refitted, the rebuilt and the plain tree"
        rows.append(dict(frame=f, refit_cost=round(cost, 4), trace_ms_refitted=round(t_refit, 4), trace_ms_rebuilt=round(t_rebuilt, 4), trace_ms_plain=round(t_plain, 4),
                         refitted_over_rebuilt=round(t_refit / t_rebuilt, 3), rebuilt_over_plain=round(t_rebuilt / t_plain, 3)))
        fresh.close(); plain.close()
    res["rows"] = rows
    if a.device_rebuild:
        sd = synth.deform(sd0, a.frames, a.kind)
        g.update_vertices(cuda(sd.verts), cuda(sd.normals))
        plain = hr.Scene(ctx, sd)
        gb = plain.gbuffer(ubo, W, H)
        fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d)
        plain.close()
        dr = dict(frame=a.frames, refit_cost_refitted=round(g.refit_cost(), 4))
        dr["trace_ms_refitted"], m_refit = trace_ms(g, fi)
        twin = hr.Scene(ctx, sd0, deformable=True)      # re-deals over the same vertices: the first call allocates, the rest are timed
        twin.update_vertices(cuda(sd.verts), cuda(sd.normals))
        for _ in range(3):
            twin.rebuild_device()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            twin.rebuild_device()
        e1.record()
        torch.cuda.synchronize()
        dr["rebuild_device_ms"] = round(e0.elapsed_time(e1) / 20, 4)
        dr["launches_per_call"] = twin.device_rebuild_counts()["launches_enqueued"] // 23
        twin.close()
        g.rebuild_device()
        dr["refit_cost_redealt"] = round(g.refit_cost(), 4)
        dr["trace_ms_redealt"], m_redealt = trace_ms(g, fi)
        fresh = hr.Scene(ctx, sd, deformable=True)
        dr["refit_cost_host_rebuilt"] = fresh.refit_cost()
        dr["trace_ms_host_rebuilt"], m_host = trace_ms(fresh, fi)
        fresh.close()
        assert np.array_equal(m_refit, m_redealt) and np.array_equal(m_refit, m_host), "masks differ between the refitted, the re-dealt and the host-rebuilt tree"
        still = hr.Scene(ctx, sd0, deformable=True)
        still.rebuild_device()
        dr["refit_cost_redealt_undecayed"] = round(still.refit_cost(), 4)
        still.close()
        res["device_rebuild"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in dr.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.rebuild()
    res["rebuild_s"] = round(time.perf_counter() - t0, 3)
    res["refit_cost_after_rebuild"] = g.refit_cost()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
