"""What extra lights cost (developer tool, GPU): at 1080p on the bench scene, in one process, the device time of hr_lights_render with 1, 4 and 16
point lights in the scene's list (lights.placed_point_lights), next to the shadow pass's trace launch (one soft shadow ray per texel for the UBO
light: the yardstick for "one ray per texel"), and of the DDGI trace launch (16 x 8 x 16 probes, 256 rays) with an empty list (k_ddgi_trace, the
kernel the parent commit launches) and with 4 lights (k_ddgi_trace_lights).  Device events around single launches, warmed; median and minimum of
--iters launches.

    python tools/lights_probe.py [--iters 20] [--counts 1 4 16] [--detail 1.0]

One JSON line; docs/EXPERIMENTS.md "Extra lights" is where its numbers go."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.probe_vis_probe import timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--counts", nargs="+", type=int, default=[1, 4, 16])
    ap.add_argument("--detail", type=float, default=1.0, help="synth.sponza_like detail")
    args = ap.parse_args()
    import torch
    from hybrid_rendering_amd import api as hr, api_gi, lights, synth, synth_env
    ctx = hr.Context(0)
    sd = synth.sponza_like(args.detail)
    lo, hi = sd.bounds()
    grid = synth_env.ddgi_uniforms(lo, hi, probe_counts=(16, 8, 16), rays_per_probe=256, normal_bias=0.1)
    f16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.float16)
    sky = synth_env.sky_cubemap(32)
    env = api_gi.environment(f16(sky.view(np.int16)), f16(synth_env.prefiltered_chain(sky, 5).view(np.int16)), 32, 5, f16(synth_env.brdf_lut(32).view(np.int16)))
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    W, H = 1920, 1080
    ubo = synth.make_ubo(synth.sponza_camera(W / H), None, synth.sponza_light())
    scene = hr.Scene(ctx, sd)
    g = scene.gbuffer(ubo, W, H)
    fi = hr.frame_inputs(g, None, ubo, 1, 1, sob_d, sr_d)
    sh, gi, lp = hr.RayTracedShadows(ctx, W, H), api_gi.DDGI(ctx, W, H, grid), lights.Lights(ctx, W, H)
    gi.render(scene, fi, env, synth_env.random_orientation(np.random.RandomState(1)))   # atlases for the infinite bounce
    out = dict(scene=sd.name, triangles=sd.n_tris, iters=args.iters, size=[W, H], lights_render={}, ddgi_trace={})
    out["shadows_trace"] = timed(lambda: sh.ray_trace(scene, fi), args.iters)
    out["ddgi_trace"]["0"] = timed(lambda: gi.ray_trace(scene, fi, env), args.iters)
    for n in args.counts:
        scene.set_lights(lights.placed_point_lights(lo, hi, n))
        torch.cuda.synchronize()
        rec = timed(lambda: lp.render(scene, fi), args.iters)
        rec["per_light_us"] = round(rec["median_us"] / n, 1)
        rec["over_shadows_trace"] = round(rec["median_us"] / out["shadows_trace"]["median_us"], 2)
        out["lights_render"][str(n)] = rec
        if n == 4:
            out["ddgi_trace"]["4"] = timed(lambda: gi.ray_trace(scene, fi, env), args.iters)
            out["ddgi_trace"]["4"]["over_empty_list"] = round(out["ddgi_trace"]["4"]["median_us"] / out["ddgi_trace"]["0"]["median_us"], 3)
    lit = (lp.output()[..., :3] != 0).any(-1).float().mean()
    out["texels_lit_by_the_last_list"] = round(float(lit), 3)
    for p in (sh, gi, lp, scene):
        p.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
