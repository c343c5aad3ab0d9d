"""What emissive materials cost (developer tool, GPU): the device time of the three emissive trace kernels against the plain ones, in one process over
the bench scene, with about 1 % and about 50 % of the hits on an emitter (synth.with_emissive_twins: that share of the triangles moved to an
emissive twin of their material), and of hr_gbuffer_emissive and hr_deferred_add_emissive at 1080p and 4K next to hr_gbuffer_raycast.
`plain` is the same scene with emission switched off (the kernels the parent commit launches); `dark_emissive` is the emissive kernel with nothing
to add (constants set to zero through the device form, which the host cannot see); `emissive` adds E.  Device events around single launches, warmed;
median and minimum of --iters launches.  The DDGI emissive kernel on a flat scene runs under the CUTOUT kernels' occupancy bound (4 waves per SIMD,
the plain kernel 6): HR_CFLAGS=-DDDGI_TRACE_CUTOUT_EU=6 python -m hybrid_rendering_amd.build --variant eu6, then HR_LIBRARY=<that library>, gives
the other side of that choice.

    python tools/emission_probe.py [--iters 20] [--sizes 1920x1080 3840x2160] [--fractions 0.01 0.5] [--detail 1.0]

One JSON line; docs/EXPERIMENTS.md "Emissive materials" is where its numbers go."""
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
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--fractions", nargs="+", type=float, default=[0.01, 0.5])
    ap.add_argument("--detail", type=float, default=1.0, help="synth.sponza_like detail")
    args = ap.parse_args()
    import torch
    from hybrid_rendering_amd import api as hr, api_deferred, api_gi, api_post, api_reflections, synth, synth_env
    ctx = hr.Context(0)
    base = synth.sponza_like(args.detail)
    lo, hi = base.bounds()
    grid = synth_env.ddgi_uniforms(lo, hi, probe_counts=(16, 8, 16), rays_per_probe=256, normal_bias=0.1)
    f16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.float16)
    sky = synth_env.sky_cubemap(32)
    env = api_gi.environment(f16(sky.view(np.int16)), f16(synth_env.prefiltered_chain(sky, 5).view(np.int16)), 32, 5, f16(synth_env.brdf_lut(32).view(np.int16)))
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    light = synth.sponza_light()
    W, H = 1920, 1080
    ubo = synth.make_ubo(synth.sponza_camera(W / H), None, light)
    out = dict(scene=base.name, triangles=base.n_tris, iters=args.iters, trace_size=[W, H], fractions={}, images={})
    for fraction in args.fractions:
        sd = synth.with_emissive_twins(base, fraction)
        scene = hr.Scene(ctx, sd)
        rgb = np.ascontiguousarray(sd.materials[:, 5:8], np.float32)
        g = scene.gbuffer(ubo, W, H)
        half = hr.gbuffer_mip(g, 1)
        fi = hr.frame_inputs(g, None, ubo, 1, 1, sob_d, sr_d)
        fh = hr.frame_inputs(half, None, ubo, 1, 1, sob_d, sr_d, cur_full=g)
        gi, rf = api_gi.DDGI(ctx, W, H, grid), api_reflections.RayTracedReflections(ctx, W, H, hr.SCALE_HALF_RES)
        gt = {ind: api_post.GroundTruthPathTracer(ctx, W, H) for ind in (0, 1)}
        gt[1].params.trace_indirect, gt[1].params.max_ray_bounces = 1, 3
        gi.render(scene, fi, env, synth_env.random_orientation(np.random.RandomState(1)))   # atlases for the infinite bounce and the reflections' gather
        calls = dict(ddgi_trace=lambda: gi.ray_trace(scene, fi, env), refl_trace=lambda: rf.ray_trace(scene, fh, env, gi),
                     ground_truth=lambda: gt[0].render(scene, ubo, env), ground_truth_indirect=lambda: gt[1].render(scene, ubo, env))
        rec = {}
        states = (("plain", lambda: scene.set_emission(False, 1.0)),
                  ("dark_emissive", lambda: scene.set_emission(True, 1.0).set_emissive(torch.zeros((len(rgb), 3), dtype=torch.float32, device="cuda"))),
                  ("emissive", lambda: scene.set_emission(True, 1.0).set_emissive(rgb)))
        for state, switch in states:
            switch()
            torch.cuda.synchronize()
            for name, call in calls.items():
                rec.setdefault(name, {})[state] = timed(call, args.iters)
        for name in calls:
            for state in ("dark_emissive", "emissive"):
                rec[name][state]["over_plain"] = round(rec[name][state]["median_us"] / rec[name]["plain"]["median_us"], 3)
        # the share of the probe rays that met an emitter: radiance texels the emission changed
        scene.set_emission(False, 1.0); gi.ray_trace(scene, fi, env); torch.cuda.synchronize()
        off = gi.image(gi.IMG_RADIANCE).clone()
        scene.set_emission(True, 1.0); gi.ray_trace(scene, fi, env); torch.cuda.synchronize()
        rec["probe_rays_on_an_emitter"] = round(float((gi.image(gi.IMG_RADIANCE) != off).any(-1).float().mean()), 4)
        out["fractions"][str(fraction)] = rec
        for p in (gi, rf, gt[0], gt[1], scene):
            p.close()
    scene = hr.Scene(ctx, synth.with_emissive_twins(base, args.fractions[-1])).set_emission(True, 1.0)
    for size in args.sizes:
        W, H = (int(v) for v in size.split("x"))
        ubo = synth.make_ubo(synth.sponza_camera(W / H), None, light)
        df = api_deferred.DeferredShading(ctx, W, H)
        image = scene.emissive_image(ubo, W, H)
        out["images"][size] = dict(gbuffer_raycast=timed(lambda: scene.gbuffer(ubo, W, H), args.iters), gbuffer_emissive=timed(lambda: scene.emissive_image(ubo, W, H), args.iters),
                                   add_emissive=timed(lambda: df.add_emissive(image), args.iters))
        df.close()
    scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
