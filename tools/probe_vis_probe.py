"""What the probe-grid visualisation costs (developer tool, GPU): the device time of hr_probe_vis_render over the bench scene's G-buffer and its
16 x 8 x 16 probe grid, at 1080p and 4K, at radius = step / 8 (the lattice walk: what every preset of the reference uses) and at 0.75 * step
(overlapping spheres: every probe is tested), next to k_deferred — the composite it draws onto — in the same process.  Device events around
single launches, warmed; median and minimum of --iters launches.

    python tools/probe_vis_probe.py [--iters 30] [--sizes 1920x1080 3840x2160] [--detail 1.0]

One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, iters, warm=5):
    import torch
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)   # the device idles ~1 ms while the host enqueues what follows: no host time between the two events
        a.record()
        call()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(np.min(us)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--detail", type=float, default=1.0, help="synth.sponza_like detail")
    args = ap.parse_args()
    import torch
    from hybrid_rendering_amd import api as hr, api_deferred, api_gi, probe_vis, synth, synth_env
    ctx = hr.Context(0)
    sd = synth.sponza_like(args.detail)
    scene = hr.Scene(ctx, sd)
    lo, hi = sd.bounds()
    grid = synth_env.ddgi_uniforms(lo, hi, probe_counts=(16, 8, 16), rays_per_probe=256, normal_bias=0.1)
    step = float(grid["grid_step"].min())
    rng = np.random.RandomState(1)
    f16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.float16)
    rand16 = lambda shape, hi_: f16(rng.uniform(0.0, hi_, shape).astype(np.float16).view(np.int16))
    irr = rand16((int(grid["irradiance_texture_height"]), int(grid["irradiance_texture_width"]), 4), 4.0)
    dep = rand16((int(grid["depth_texture_height"]), int(grid["depth_texture_width"]), 2), float(grid["max_distance"]))
    sky = synth_env.sky_cubemap(32)
    env = api_gi.environment(f16(sky.view(np.int16)), f16(synth_env.prefiltered_chain(sky, 5).view(np.int16)), 32, 5, f16(synth_env.brdf_lut(32).view(np.int16)))
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    out = dict(grid=[16, 8, 16], step=round(step, 3), iters=args.iters, sizes={})
    for size in args.sizes:
        W, H = (int(v) for v in size.split("x"))
        ubo = synth.make_ubo(synth.sponza_camera(W / H), None, synth.sponza_light())
        g = scene.gbuffer(ubo, W, H)
        fi = hr.frame_inputs(g, None, ubo, 0, 0, sob_d, sr_d)
        df = api_deferred.DeferredShading(ctx, W, H)
        df.set_sh9(synth_env.sh9_from_cubemap(sky))
        # the composite with every input switched on, over stand-in pass outputs: its time does not depend on what they hold
        shadow, ao, refl, gi = rand16((H, W), 1.0), rand16((H, W), 1.0), rand16((H, W, 4), 2.0), rand16((H, W, 4), 2.0)
        rec = dict(k_deferred=timed(lambda: df.render(fi, env, shadow=shadow, ao=ao, reflections=refl, gi=gi), args.iters))
        color = df.output()
        depth_out = torch.empty_like(g["depth"])
        ids = torch.empty((H, W), dtype=torch.int32, device="cuda")
        for label, radius, what in (("walk_r_step_8", step / 8.0, 0), ("walk_r_step_8_depth_atlas", step / 8.0, 1), ("walk_r_step_2", step / 2.0, 0), ("all_probes_r_0.75_step", 0.75 * step, 0)):
            call = lambda: probe_vis.render(ctx, ubo, grid, irr, g["depth"], color, depth_atlas=dep, radius=radius, what=what, depth_out=depth_out, probe_id_out=ids)
            rec[label] = timed(call, args.iters if radius <= step / 2.0 else max(3, args.iters // 6), warm=5 if radius <= step / 2.0 else 1)
            rec[label]["drawn"] = round(float((ids >= 0).float().mean()), 4)
            rec[label]["share_of_k_deferred"] = round(rec[label]["median_us"] / rec["k_deferred"]["median_us"], 3)
        out["sizes"][size] = rec
        df.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
