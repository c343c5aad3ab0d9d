"""What alpha-tested cutout materials cost (developer tool): per-stage times of the shadows and AO passes on the hard tier of synth.sponza_like
with its foliage material (synth.FOLIAGE_MATERIAL) turned into a cutout through synth.with_leaf_cutout, for three cases —
    parent   a library built from the parent commit (--parent-lib PATH; skipped without it), the scene opaque;
    zeros    this tree's library, every cutoff 0 (the CUTOUT = false instantiations: must time like `parent`);
    cutout   this tree's library, the foliage cutoff on (the CUTOUT instantiations)
— each in a process of its own, `--rounds` times alternating, one JSON line per (round, case) with the stage times in microseconds.  The three
cases trace from the same opaque G-buffer (RAY_PRIMARY is forced opaque), so the numbers compare the walks of the shadow and AO rays alone.

    python tools/cutout_probe.py [--width 1920 --height 1080 --frames 30 --rounds 3] [--parent-lib /path/to/parent/libhybrid_rendering_amd.so]
    python tools/cutout_probe.py --rejection-rate      (no GPU: the rejection rate per shadow ray, counted on the CPU reference)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_case(args):
    import numpy as np
    import torch
    from hybrid_rendering_amd import api as hr, synth
    W, H = args.width, args.height
    sd = synth.with_leaf_cutout(synth.sponza_like(1.0, tier="hard"))
    ctx = hr.Context(0)
    scene = hr.Scene(ctx, sd)
    if args.case == "zeros":
        scene.set_alpha_cutoffs(np.zeros(len(sd.materials), np.float32))
    elif args.case == "cutout":
        scene.set_alpha_cutoffs(sd.alpha_cutoffs)
    light = synth.sponza_hard_light()
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(5)]
    ubos = [synth.make_ubo(cams[i + 1], cams[i], light) for i in range(4)]
    if args.case != "parent":
        scene.set_ray_class_opaque(hr.RAY_PRIMARY, True)   # the three cases trace from the same (opaque) G-buffer
    gbs = [scene.gbuffer(u, W, H) for u in ubos]
    zbp = synth.z_buffer_params()
    out = dict(case=args.case, width=W, height=H, library=hr.LIB_PATH)
    for name, make in (("shadows", lambda: hr.RayTracedShadows(ctx, W, H)), ("ao", lambda: hr.RayTracedAO(ctx, W, H, 0))):
        p = make()
        p.params.exact = 0
        fis = [hr.frame_inputs(gbs[k % 4], gbs[(k - 1) % 4], ubos[k % 4], k, k & 1, sob_d, sr_d, z_buffer_params=zbp) for k in range(8)]
        for k in range(8):
            fis[k].num_frames = k
            p.render(scene, fis[k])
        torch.cuda.synchronize()
        p.set_profiling(True)
        for k in range(8, 8 + args.frames):
            fis[k % 8].num_frames = k
            p.render(scene, fis[k % 8])
        torch.cuda.synchronize()
        out[name] = {stage: round(ms * 1e3, 1) for stage, ms, _ in p.stage_times()}   # us, averaged over the frames
        out[name + "_rays"] = int(p.ray_count())
        p.close()
    print(json.dumps(out), flush=True)


def rejection_rate(args):
    """No GPU.  Camera rays of a (width / 8) x (height / 8) frame through the oracle, then from every visible point a shadow ray towards the centre of the
    hard tier's sun, walked hit by hit on the CPU: closest hit, the numpy float32 replay of csrc/cutout.h on it (tests/cutout_cases.py), and on from a
    rejected hit (t_min = t * (1 + 2^-21): the oracle's own t would be found again).  Prints the share of shadow rays that meet at least one rejected
    hit, the rejected hits per ray, and the occluded share with the scene opaque and with the cutout."""
    import numpy as np
    from hybrid_rendering_amd import synth
    from oracle import pyoracle as po
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cutout_cases as cc
    po.build(); po.lib()
    sd = synth.with_leaf_cutout(synth.sponza_like(1.0, tier="hard"))
    osc = po.Scene(synth.SceneData(sd.verts, sd.normals, sd.tri_material, sd.tri_mesh_id, sd.materials))
    w, h = args.width // 8, args.height // 8
    cam = synth.sponza_camera(w / h, frame=1, dolly=0.5)
    eye = np.asarray(cam.eye, np.float64)
    fwd = np.asarray(cam.target, np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, (0.0, 1.0, 0.0)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    th = np.tan(np.radians(cam.fov) / 2)
    yy, xx = np.mgrid[0:h, 0:w]
    d = fwd + ((2 * (xx.ravel() + 0.5) / w - 1) * th * w / h)[:, None] * right + ((1 - 2 * (yy.ravel() + 0.5) / h) * th)[:, None] * up
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((w * h, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = eye, 1e4, d, 0.001
    tuv, prim = osc.closest_hit(r)
    seen = prim >= 0
    L = np.asarray(synth.sponza_hard_light(), np.float32).reshape(-1)[0:3].astype(np.float64)
    L /= np.linalg.norm(L)
    s = np.zeros((int(seen.sum()), 8), np.float32)
    s[:, 0:3] = r[seen, 0:3] + r[seen, 4:7] * tuv[seen, 0:1] + L * 0.1
    s[:, 3], s[:, 4:7], s[:, 7] = 1e4, L, 0.01
    opaque = osc.any_hit(s) != 0
    rejected, occluded = np.zeros(len(s), np.int64), np.zeros(len(s), bool)
    live, steps = np.arange(len(s)), 0
    while len(live) and steps < 256:
        steps += 1
        tuv, prim = osc.closest_hit(s[live])
        hit = prim >= 0
        live, tuv, prim = live[hit], tuv[hit], prim[hit]
        acc = np.ones(len(live), bool)
        for m in np.flatnonzero(sd.alpha_cutoffs > 0):
            k = np.flatnonzero(sd.tri_material[prim] == m)
            q = sd.uvs[prim[k]]
            u, v = tuv[k, 1], tuv[k, 2]
            b0 = np.float32(1.0) - u - v
            tu, tv = (q[:, 0, 0] * b0 + q[:, 1, 0] * u) + q[:, 2, 0] * v, (q[:, 0, 1] * b0 + q[:, 1, 1] * u) + q[:, 2, 1] * v
            acc[k] = ~(cc.texture_alpha(sd.textures[int(sd.material_textures[m][0])], tu, tv) < np.float32(sd.alpha_cutoffs[m]))
        occluded[live[acc]] = True
        rejected[live[~acc]] += 1
        s[live[~acc], 7] = tuv[~acc, 0] * np.float32(1.0 + 2.0 ** -21)
        live = live[~acc]
    print(json.dumps(dict(case="rejection_rate", frame=f"{w}x{h}", shadow_rays=len(s), rays_meeting_a_rejected_hit=round(float((rejected > 0).mean()), 4),
                          rejected_hits_per_ray=round(float(rejected.mean()), 4), most_rejected_hits_on_one_ray=int(rejected.max()),
                          occluded_opaque=round(float(opaque.mean()), 4), occluded_cutout=round(float(occluded.mean()), 4), unfinished_rays=int(len(live)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--case", default="", choices=["", "parent", "zeros", "cutout"])
    ap.add_argument("--rejection-rate", action="store_true", help="no GPU: how many shadow rays of the view meet a rejected hit, counted on the CPU reference")
    args = ap.parse_args()
    if args.rejection_rate:
        return rejection_rate(args)
    if args.case:
        return one_case(args)
    cases = (["parent"] if args.parent_lib else []) + ["zeros", "cutout"]
    for r in range(args.rounds):
        for case in cases:
            env = dict(os.environ)
            if case == "parent":
                env["HR_LIBRARY"] = args.parent_lib
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--width", str(args.width), "--height", str(args.height),
                                 "--frames", str(args.frames)], env=env, timeout=300).returncode
            if rc != 0:
                sys.exit(f"case {case} of round {r} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
