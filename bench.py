#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X-native ray-trace + denoise hot path.

One "step" = one frame of RayTracedShadows::render (1 spp soft-shadow trace + SVGF temporal + 4 x a-trous) on synthetic 1080p
G-buffers of the procedural Sponza-like scene (~278k triangles), inputs resident in HBM (BASELINE.json configs[1]), in the
shipping arithmetic mode (hr_shadows_params.exact = 0: bit-exact masks, fp16 images within the stated tolerance; the bit-for-bit
parity mode is timed next to it and reported as `exact_mode`).  Prints ONE JSON line (see the driver contract).

    python bench.py --gpus 1 --steps 200 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times ONE region of exactly `--steps` steps, counts the rays of the frames after it (`value` divides
them) and prints the line.  --dump-outputs DIR writes what the last timed step computed (denoised.npy, shadow_mask.npy) first.

With --full, besides the headline the line carries (outside the timed region, short runs): the same region repeated until >= 5 s are
timed (`timed_repeats`, `ms_per_step_median`), per-kernel HIP-event times (`stages`), the other arithmetic mode (`exact_mode`), and
  passes       N = 1: BASELINE configs[2], [3] and the passes of [4] on one GPU — AO 4 spp, half-res reflections, DDGI 16x8x16x256, the
               whole hybrid frame at 1080p and at 4K: ms, Mrays/s, frames/s and, per kernel, the HIP-event time and the fraction of the
               8 TB/s HBM roofline its ALGORITHMIC bytes amount to;
  hybrid_4k    N > 1: BASELINE configs[4] itself — ONE 3840x2160 hybrid frame row-tiled over the N GPUs (strong scaling), max over ranks;
  roofline     dominant kernel of the headline; `frac` = algorithmic bytes / time / peak, `dram_frac` = rocprofv3 PMC traffic / time / peak
               and `bound` = what the committed SQ counters of this build say limits it (profiles/, tools/profile_round.sh);
  cpu_baseline the SAME ray batch replayed through the oracle's scalar BVH traversal on the host cores (`trace_replay`) and the oracle's
               denoise chain timed separately (`denoise_ms`), BASELINE.md §3.

N > 1 (weak scaling of the headline): the SAME view is rendered with N times the pixels — 1920*sqrt(N) x 1080*sqrt(N), rounded to
multiples of 8 — so rays and pixels per frame grow with N while the content statistics stay those of the N = 1 frame.
The frame is row-tiled, one band per GPU; band boundaries are chosen from a calibration frame so that every band
carries the same share of the cost model  pixels + 1.8 * rays  (tiling.balanced_bounds: sky rows fire no ray, the
floor fires one per pixel — equal-height bands would leave most GPUs idle).  Every band re-traces / re-filters 24 halo
rows locally and, once per frame, exchanges the 40 history rows next to each band boundary with its neighbours over
RCCL (hybrid_rendering_amd/tiling.py), overlapped with the next frame's trace; band rows are bit-identical to the
single-GPU result in exact mode (tests/test_gpu_tiling.py).  `value` counts only the rays of band rows (halo work is overhead).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import sys
import threading
import time

import numpy as np

# kernel arguments in device memory (the HIP runtime's default on this image; measured: headline 0.196 ms with it, 0.205 ms without —
# the pass kernels take 200-500 byte argument blocks).  Must be set before the HIP runtime initialises.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import bench_report
from bench_report import (HBM_PEAK_GBS, NODE_BYTES, TRI_BYTES, LINE_LIMIT, DETAIL_FILE, kernel_of, norm_kernel, load_profile, classify, compact_line,
                          binding_frac, pass_roofline, kernel_entries)

def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--detail", type=float, default=1.0, help="scene tessellation (1.0 = ~278k triangles)")
    ap.add_argument("--tier", default="standard", choices=["standard", "hard"], help="hard: the ~2.5 M triangle scene with layered fabric, foliage cards and a grazing sun as the headline workload")
    ap.add_argument("--obj", default=None, help="Wavefront OBJ (+MTL) to render instead of the procedural scene (hybrid_rendering_amd/assets.py)")
    ap.add_argument("--ring", type=int, default=8, help="distinct camera positions cycled through")
    ap.add_argument("--exact", type=int, default=0, help="1: time the bit-for-bit parity arithmetic as the headline instead of the tolerance mode")
    ap.add_argument("--full", action="store_true", help="everything besides the headline: repeated timed regions, per-kernel times and roofline, the other "
                    "arithmetic mode, the `passes` / `hybrid_4k` blocks, the CPU baseline, the `comm` block of N > 1")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-passes", action="store_true", help="with --full: skip the `passes` / `hybrid_4k` blocks (profiling runs)")
    ap.add_argument("--cpu-frames", type=int, default=4)
    return ap.parse_args()


# ---- one JSON line, whatever happens (first multi-GPU contact must not be able to end without a parseable line) -------------
PROGRESS = {"stage": "start", "rank": 0, "world": 1}     # where this rank is (the watchdog prints it)
PARTIAL = {}                                             # rank 0: the line as far as it is known
_printed = threading.Event()


def stage(name):
    PROGRESS["stage"] = name


_LINE_FD = None   # isolate_stdout(): the descriptor the ONE line goes to


def isolate_stdout():
    """stdout must carry exactly one line, and it must be the last thing on it.  Libraries write there behind Python's back — RCCL prints a five-line
    banner through C stdio at its first communicator, which sits in libc's buffer until the process EXITS, i.e. lands after the JSON line of a
    `--gpus N` run (and every other rank's copy lands in the launcher's merged stdout whenever that rank exits).  So every rank points descriptor 1
    at stderr for the whole run and keeps the real stdout aside for emit()."""
    global _LINE_FD
    if _LINE_FD is not None:
        return
    try:
        sys.stdout.flush()
        _LINE_FD = os.dup(1)
        os.dup2(2, 1)
    except OSError:
        _LINE_FD = None


def flush_c_stdio():
    """whatever libraries have written through C stdio so far leaves libc's buffer NOW (before the line), not when the process exits (after it) —
    for a driver that reads stdout and stderr as one stream"""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def emit(out):
    """prints the bench line once per process: the full record goes to bench_detail.json (next to this script and, when that directory exists,
    under gpurun_out/) and to stderr; stdout gets ONE compact line (compact_line)"""
    if _printed.is_set():
        return
    _printed.set()
    full = json.dumps(out)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, DETAIL_FILE), "w") as f:
                    f.write(full + "\n")
        except OSError:
            pass
    print("[bench detail] " + full, file=sys.stderr, flush=True)
    try:
        line = json.dumps(compact_line(out))
    except Exception as e:   # never lose the line to its own summariser
        line = json.dumps({**stub_line_from(out), "error": f"compact_line failed: {e!r}"[:300]})
    sys.stdout.flush()
    flush_c_stdio()
    if _LINE_FD is not None:
        os.write(_LINE_FD, (line + "\n").encode())
    else:
        print(line, flush=True)


def stub_line_from(out):
    return {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")}


def stub_line(args, world, error):
    """the contract's fields with no measurement in them: what rank 0 prints when nothing could be measured"""
    return {"metric": "shadow Mrays/s over the fully denoised frame (1 spp trace + SVGF temporal + 4x a-trous)", "value": 0.0, "unit": "Mrays/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic", "config": {"workload": f"{args.width}x{args.height} procedural Sponza-like ray-traced shadows 1spp + SVGF denoise"}, "error": error}


def start_watchdog(args, rank, world):
    """HR_BENCH_TIMEOUT_S (default 900): a rank that has not finished by then says where it is (stage, last collective it posted), rank 0 prints
    the line as far as it is known with `error`, and the process exits with code 3 instead of hanging in a collective its peer never posts."""
    limit = float(os.environ.get("HR_BENCH_TIMEOUT_S", "900"))

    def fire():
        last = None
        try:
            from hybrid_rendering_amd import tiling
            last = dict(tiling.LAST_COLLECTIVE)
        except Exception:
            pass
        msg = f"watchdog: rank {rank}/{world} not finished after {limit:.0f} s at stage '{PROGRESS['stage']}'; last collective posted: {last}"
        print("[bench] " + msg, file=sys.stderr, flush=True)
        if rank == 0:
            out = dict(PARTIAL) if PARTIAL else stub_line(args, world, msg)
            out["error"] = msg
            out.setdefault("comm", {})
            if isinstance(out["comm"], dict):
                out["comm"].update({"error": msg, "stage": PROGRESS["stage"], "last_collective": last})
            emit(out)
        os._exit(3)
    t = threading.Timer(limit, fire)
    t.daemon = True
    t.start()
    return t


def main():
    args = parse()
    isolate_stdout()
    if os.environ.get("HR_BENCH_TEST_C_STDOUT"):   # test hook (tests/test_bench_robustness.py): what a library's C stdio does — buffered, flushed when the process exits
        import ctypes
        ctypes.CDLL(None).printf(b"a library's banner, written through C stdio\n")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    PROGRESS.update(rank=rank, world=world)
    wd = start_watchdog(args, rank, world)
    import torch
    import torch.distributed as dist
    if world != args.gpus and rank == 0:
        print(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}; using WORLD_SIZE", file=sys.stderr)
    if os.environ.get("HR_FORCE_DEVICE") is not None:  # developer switch: several ranks on ONE GPU (functional test of the N>1 path)
        local_rank = int(os.environ["HR_FORCE_DEVICE"])
    comm_error = None
    try:
        torch.cuda.set_device(local_rank)
        if world > 1:
            stage("init_process_group")
            import datetime
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            # a collective timeout LONGER than the watchdog's: the watchdog (which prints the line) fires first
            dist.init_process_group(os.environ.get("HR_DIST_BACKEND", "nccl"),   # "nccl" is RCCL on ROCm
                                    timeout=datetime.timedelta(seconds=float(os.environ.get("HR_BENCH_TIMEOUT_S", "900")) + 600))
            if os.environ.get("HR_BENCH_FAIL_AT") == "init":   # test hook (tests/test_bench_robustness.py)
                raise RuntimeError("HR_BENCH_FAIL_AT=init")
    except Exception as e:
        comm_error = f"{PROGRESS['stage']}: {e!r}"[:400]
    out = None
    if comm_error is None:
        try:
            out = run(args, torch, dist, rank, world, local_rank)
        except Exception as e:
            import traceback
            traceback.print_exc()
            if world == 1:
                out = dict(PARTIAL) if PARTIAL else stub_line(args, world, "")
                out["error"] = f"{PROGRESS['stage']}: {e!r}"[:400]
                emit(out)
                sys.exit(1)
            comm_error = f"{PROGRESS['stage']}: {e!r}"[:400]
    if comm_error is not None:
        # the distributed run failed: rank 0 reports the N = 1-equivalent local numbers next to the error, the other ranks leave quietly
        # (exit code 0: a launcher that tears the job down on the first non-zero exit would take rank 0 with it before it has printed)
        print(f"[bench] rank {rank}: distributed run failed ({comm_error})" + ("; falling back to a local single-GPU run" if rank == 0 else "; leaving"), file=sys.stderr, flush=True)
        if rank != 0:
            os._exit(0)
        seen = PROGRESS.get("ranks_seen", 1)
        try:
            stage("local_fallback")
            out = run(args, torch, None, 0, 1, local_rank)
        except Exception as e:
            out = dict(PARTIAL) if PARTIAL else stub_line(args, 1, "")
            out["error"] = f"local fallback after the distributed failure also failed: {e!r}"[:400]
        out["requested_gpus"] = world
        out.setdefault("error", f"distributed run failed ({comm_error}); every number on this line is rank 0's LOCAL single-GPU result (n_gpus = 1)")   # visible at top level
        out["comm"] = {"error": comm_error, "ranks_seen": seen, "backend": os.environ.get("HR_DIST_BACKEND", "nccl"),
                       "note": "the distributed run could not start / complete; `value` and everything else on this line are rank 0's LOCAL single-GPU numbers (n_gpus = 1)"}
    wd.cancel()
    flush_c_stdio()
    if world > 1 and comm_error is None:
        try:
            dist.barrier()   # every rank has emptied its C stdio buffer before rank 0 writes the line
        except Exception:
            pass
    if rank == 0:
        emit(out)
    if world > 1 and comm_error is None:
        try:
            dist.destroy_process_group()
        except Exception:
            pass
    if comm_error is not None:
        os._exit(0)   # no orderly teardown of a process group that never worked


def run(args, torch, dist, rank, world, local_rank):
    """the bench proper -> the line (a dict); world == 1 never touches torch.distributed"""
    from hybrid_rendering_amd import api as hr
    from hybrid_rendering_amd import synth, tiling
    from hybrid_rendering_amd.frame import HybridFrame

    # N x the pixels of the N = 1 frame, same aspect and view (multiples of 8: tile / band alignment)
    sc = math.sqrt(world)
    W, H = (int(round(args.width * sc / 8)) * 8, int(round(args.height * sc / 8)) * 8) if world > 1 else (args.width, args.height)
    if args.obj:
        from hybrid_rendering_amd import assets
        sd = assets.load_obj(args.obj)
        scene_name = f"{os.path.basename(args.obj)}"
    else:
        sd = synth.sponza_like(args.detail, tier=args.tier)
        scene_name = "procedural Sponza-like" + (" (hard tier: layered fabric, foliage cards, grazing sun)" if args.tier == "hard" else "")
    stage("scene")
    ctx = hr.Context(local_rank)
    scene = hr.Scene(ctx, sd)
    light = synth.sponza_hard_light() if args.tier == "hard" else synth.sponza_light()
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    exact = 1 if args.exact else 0

    # ring of camera positions (dolly 0.5 units/frame)
    R = max(2, args.ring)
    cam_of = (lambda f: synth.camera_for_bounds(sd.bounds(), W / H, frame=f, dolly=0.5)) if args.obj else (lambda f: synth.sponza_camera(W / H, frame=f, dolly=0.5))
    cams = [cam_of(f) for f in range(R + 1)]
    # G-buffers: ring position i rendered with prev = i-1 (forward sweep) and with prev = i+1 (backward sweep)
    gbs = {}
    ubos = {}
    for i in range(R):
        for direction, j in (("f", i - 1 if i > 0 else 0), ("b", i + 1)):
            ubo = synth.make_ubo(cams[i], cams[j], light)
            ubos[(i, direction)] = ubo
            gbs[(i, direction)] = scene.gbuffer(ubo, W, H)
    torch.cuda.synchronize()

    # sequence of (cur, prev) keys: 0f,1f,...,R-1f, R-2b, ..., 0b, 1f, ...
    seq = [(i, "f") for i in range(R)] + [(i, "b") for i in range(R - 2, -1, -1)]
    seq = seq[1:] if len(seq) > 1 else seq

    def inputs_for(k):
        key = seq[k % len(seq)]
        pk = seq[(k - 1) % len(seq)]
        return hr.frame_inputs(gbs[key], gbs[pk], ubos[key], k, k & 1, sob_d, sr_d)

    cycle = [inputs_for(k) for k in range(len(seq) * 2)]  # even length: ping_pong parity preserved when cycling
    bounds = None
    if world > 1:
        stage("calibration")
        if os.environ.get("HR_BENCH_FAIL_AT") == "calibration":   # test hook
            raise RuntimeError("HR_BENCH_FAIL_AT=calibration")
        seen = torch.ones(1, dtype=torch.int64, device="cuda")
        dist.all_reduce(seen, op=dist.ReduceOp.SUM)               # first collective: how many ranks the backend really connects
        PROGRESS["ranks_seen"] = int(seen.item())
        # calibration (outside the timed region, identical on every rank): rays per tile row of the whole frame + geometry
        # pixels per tile row -> band boundaries of equal modelled cost (tiling.shadow_cost_per_tile_row)
        cal = hr.RayTracedShadows(ctx, W, H)
        cal.ray_trace(scene, cycle[0])
        cost = tiling.shadow_cost_per_tile_row(gbs[seq[0]]["depth"], cal.tile_ray_counts())
        cal.close()
        bounds = tiling.balanced_bounds(cost, world, H)
        tb = torch.tensor(bounds, dtype=torch.int64, device="cuda")
        dist.broadcast(tb, src=0)      # belt and braces: every rank uses rank 0's partition
        bounds = [int(v) for v in tb.cpu()]

    def barrier():
        if world > 1:
            dist.barrier()

    def timed_run(tiled, steps, warmup):
        def step(k):
            fi = cycle[k % len(cycle)]
            fi.num_frames = k
            tiled.render(scene, fi)
        # frames in flight: the host enqueues a step in ~40 us, the GPU needs 200; left alone it runs a thousand launches ahead, and
        # past some depth the HIP queue makes the host wait in coarse steps (seen on the hybrid frame: sporadic +1 ms per frame in a
        # 30-frame run).  A renderer keeps a few frames in flight; so does this loop: before step k the host waits for step k - 32,
        # which the GPU finished long ago — the GPU never idles.
        fences = [torch.cuda.Event() for _ in range(4)]

        def paced(k):
            if k % 8:                       # a fence every 8th step (an event record costs the stream ~2 us): <= 32 steps in flight
                return step(k)
            f = fences[(k // 8) % len(fences)]
            if k >= 8 * len(fences):
                f.synchronize()
            step(k)
            f.record()
        for k in range(warmup):
            paced(k)

        def region(k_first):
            """EXACTLY `steps` steps between barrier + synchronize on both sides; max over ranks"""
            torch.cuda.synchronize()
            barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(k_first, k_first + steps):
                paced(k)
            torch.cuda.synchronize()
            barrier()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([el], dtype=torch.float64, device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el = float(t.item())
            return el
        timed_run.region = region
        return region(warmup), step      # ONE region of exactly `steps` steps

    def repeat_regions(region, first, k_first, steps, min_total_s=5.0):
        """--full: a region of K steps of a ~0.2 ms frame lasts a few ms and one host hiccup is a large share of it, so the same region (same K
        steps, same brackets) is repeated until >= 5 s have been timed in total and the MEDIAN region is reported beside the headline
        (`timed_repeats`, VERDICT r3 #5d); one region if K steps already take that long"""
        els = [first]
        n_rep = int(min(2500, max(1, math.ceil(min_total_s / max(first, 1e-6)))))
        if world > 1:   # every rank repeats the same number of times
            t = torch.tensor([n_rep], dtype=torch.int64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            n_rep = int(t.item())
        for r in range(1, n_rep):
            els.append(region(k_first + r * steps))
        return {"timed_repeats": len(els), "timed_region_ms": [round(e * 1e3, 3) for e in els][:16], "timed_total_ms": round(sum(els) * 1e3, 2),
                "ms_per_step_median": round(float(np.median(els)) / steps * 1e3, 4)}

    # ------------------------------------------------------------------------------------------------ the timed region (headline)
    stage("headline")
    tiled = tiling.TiledShadows(ctx, W, H, rank, world, bounds=bounds)
    tiled.params.exact = exact
    shadows = tiled.pass_
    b0, b1 = tiled.b0, tiled.b1
    # the GPU leaves its idle clocks before the timed pass warms up: a scratch pass (its own history, no collectives) renders the frame cycle
    # for 0.3 s.  The timed pass's state, and so what its last step computes, does not depend on it; without it the first region after a
    # short warm-up runs ~0.7 % slower than the regions after it.
    spin = hr.RayTracedShadows(ctx, W, H)
    spin.params.exact = exact
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            fi = cycle[k % len(cycle)]
            fi.num_frames = k
            spin.render(scene, fi)
            k += 1
        torch.cuda.synchronize()
    spin.close()
    elapsed, step = timed_run(tiled, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        stage("dump_outputs")
        dump_outputs(args.dump_outputs, torch, hr, tiled)
    timing = {}
    if args.full:
        stage("repeats")
        timing = repeat_regions(timed_run.region, elapsed, args.warmup, args.steps)
    stage("ray_count")

    # ---- ray counts of the frames after the timed region (`value` divides them); --full: per-kernel HIP events on the launch stream on the same
    # frames (same stream, same frame cycle: 12 event records per ~0.2 ms frame inside the timed region cost 18 % of the throughput; the per-kernel
    # averages agree within 1.5 % either way, and rocprofv3 agrees with both — DESIGN.md §5)
    acc = {}
    rays_total, n_prof = 0, min(args.steps, 60)
    k0 = args.warmup + args.steps
    shadows.set_profiling(args.full)
    for k in range(k0, k0 + n_prof):
        step(k)
        rays_total += shadows.ray_count()
        if args.full:
            for name, ms, nbytes in shadows.stage_times():
                a = acc.setdefault(name, [0.0, nbytes])
                a[0] += ms / n_prof
    shadows.set_profiling(False)
    rays_per_frame = rays_total / n_prof
    if world > 1:
        # useful rays = rays of the band rows only: count them with a halo-free pass on the same inputs
        counter = hr.RayTracedShadows(ctx, W, H, hr.SCALE_FULL_RES, band=(b0, b1, 0, 0))
        tot = 0
        for k in range(k0, k0 + 8):
            fi = cycle[k % len(cycle)]
            fi.num_frames = k
            counter.ray_trace(scene, fi)
            tot += counter.ray_count()
        rays_per_frame = tot / 8
        counter.close()
    px = W * (b1 - b0)
    total_rays = rays_per_frame * args.steps * world
    if world > 1:
        t = torch.tensor([rays_per_frame], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        total_rays = float(t.item()) * args.steps
    ms_per_step = elapsed / args.steps * 1e3
    value = total_rays / elapsed / 1e6
    out = {
        "metric": "shadow Mrays/s over the fully denoised frame (1 spp trace + SVGF temporal + 4x a-trous)",
        "value": round(value, 2), "unit": "Mrays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{W}x{H} {scene_name} ({sd.n_tris} tris) ray-traced shadows 1spp + SVGF denoise"
                               + (f", {world}x the pixels of 1920x1080 (same view), row-tiled into {world} cost-balanced bands" if world > 1 else ""),
                   "math": ("exact=1: every stage image bit-identical to the oracle" if exact else
                            "exact=0 (shipping mode): masks / ray counts bit-exact, fp16 images within tolerance (tests/test_gpu_tolerance.py)"),
                   "trace_launch_order": "blockIdx" if os.environ.get("HR_TILE_ORDER") == "0" else "heaviest tiles of the last frame first (csrc/tile_order.h)",
                   "rays_per_frame_per_gpu": int(rays_per_frame), "pixels_per_gpu": px, "bvh_nodes": int(scene.info.n_nodes)},
        "timing_note": "ms_per_step = one timed region of exactly `steps` steps (barrier + synchronize on both sides)"
                       + ("; ms_per_step_median = the median of `timed_repeats` such regions, repeated until >= 5 s are timed in total" if args.full else ""),
        "denoised_frames_per_s": round(args.steps / elapsed, 2),                  # frames of W x H (the whole tiled frame)
        "denoised_1080p_equiv_per_s": round(W * H / (args.width * args.height) * args.steps / elapsed, 2),
    }
    if not args.full:
        stage("done")
        return out

    # ---- --full: everything below is reported next to the headline, never part of it
    out.update(timing)
    stage("per_kernel")
    stages = {n: dict(ms=v[0], bytes=v[1]) for n, v in acc.items()}
    # instrumented trace (node visits / triangle tests) on a few frames of the cycle
    # (VERDICT r4 #1a) the counts `frac` divides are those of the TIMED kernel: occluder cache ON, in the state the previous frame of the
    # cycle left it in (hr_shadows_trace_stats_timed).  The full walk (cache bypassed: comparable between frames, builds and rounds) is
    # reported beside it.  Frame kk is counted, then rendered, so that frame kk + 1 meets the cache a timed frame meets.
    nn = nt = nr = wn = wt = wr = 0
    kk0 = k0 + n_prof
    for kk in range(kk0, kk0 + 4):
        fi = cycle[kk % len(cycle)]
        fi.num_frames = kk
        r, a, b = shadows.trace_stats(scene, fi)                    # the walk
        wr, wn, wt = wr + r, wn + a, wt + b
        r, a, b = shadows.trace_stats(scene, fi, timed=True)        # what the timed kernel does on this frame
        nr, nn, nt = nr + r, nn + a, nt + b
        step(kk)
    nodes_per_ray, tris_per_ray = nn / max(nr, 1), nt / max(nr, 1)
    walk_nodes_per_ray, walk_tris_per_ray = wn / max(wr, 1), wt / max(wr, 1)
    trace_bytes = px * 12.125 + rays_per_frame * (nodes_per_ray * NODE_BYTES + tris_per_ray * TRI_BYTES)
    walk_bytes = px * 12.125 + rays_per_frame * (walk_nodes_per_ray * NODE_BYTES + walk_tris_per_ray * TRI_BYTES)
    if "ray_trace" in stages:
        stages["ray_trace"]["bytes"] = int(trace_bytes)
    prof = load_profile()
    profiled_config = world == 1 and (W, H) == (1920, 1080) and not args.obj and args.tier == "standard"
    if not profiled_config:
        # another frame size / scene than the profiled one: neither the per-launch counter traffic nor the durations carry over
        prof = dict(prof, traffic={}, traffic_lo={}, avg_us={}, sq={})
    for n, s in stages.items():
        kern = kernel_of("shadows", n, exact) or n
        s.update(classify(prof, kern, s["ms"], s["bytes"], gather=(n == "ray_trace")))
        s["GBps"] = s["bytes"] / (s["ms"] * 1e-3) / 1e9 if s["ms"] > 0 else 0.0

    comm_info = None
    if world > 1:
        # what the driver's SCALE record needs to tell compute from communication: how many ranks RCCL really saw, the band cut, and
        # the cost of one history exchange posted and waited for back to back (max over ranks; in the frame it hides under the next trace)
        seen = torch.ones(1, dtype=torch.int64, device="cuda")
        dist.all_reduce(seen, op=dist.ReduceOp.SUM)
        ex = torch.tensor([tiled.time_exchange(20)], dtype=torch.float64, device="cuda")
        dist.all_reduce(ex, op=dist.ReduceOp.MAX)
        comm_info = bench_report.comm_block(dist.get_backend(), seen.item(), bounds, tiled.history_rows, ex.item(), W)
    dom = max(stages.items(), key=lambda kv: kv[1]["ms"])
    out["config"].update({"nodes_per_ray": round(nodes_per_ray, 2), "tris_per_ray": round(tris_per_ray, 2),
                          "nodes_per_ray_full_walk": round(walk_nodes_per_ray, 2), "tris_per_ray_full_walk": round(walk_tris_per_ray, 2)})
    out.update({
        "trace_only_Mrays_per_s": round(rays_per_frame / (stages["ray_trace"]["ms"] * 1e-3) / 1e6, 2) if "ray_trace" in stages else None,
        "roofline": {"kernel": dom[0], "kernel_name": dom[1].get("kernel"), "bound": dom[1].get("bound") or "latency", "achieved": round(dom[1]["GBps"], 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": dom[1]["frac"], "traffic": dom[1].get("traffic"), "traffic_lo": dom[1].get("traffic_lo"), "dram_frac": dom[1].get("dram_frac"),
                     "valu_issue_frac": dom[1].get("valu_issue_frac"), "lane_utilisation": dom[1].get("lane_utilisation"), "valu_frac": dom[1].get("valu_frac"),
                     "binding_frac": binding_frac(dom[1]),
                     # a trace kernel's algorithmic bytes are REQUESTED bytes: every lane's 80 B node / 48 B triangle fetch, most of them L1 / L2 hits
                     # (the tree is ~17 MB) — `frac` is SURVEY 8d's figure, not an HBM share; dram_frac is (VERDICT r4 #1b)
                     "frac_is_requested_bytes": dom[0] == "ray_trace",
                     "frac_kind": "requested_bytes" if dom[0] == "ray_trace" else "hbm_algorithmic",
                     "l2_frac": (round(dom[1]["bytes"] / (dom[1]["ms"] * 1e-3) / 1e9 / bench_report.L2_PEAK_GBS, 4) if dom[0] == "ray_trace" and dom[1]["ms"] > 0 else None),
                     "frac_full_walk": (round(walk_bytes / (dom[1]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if dom[0] == "ray_trace" and dom[1]["ms"] > 0 else None),
                     "binding_note": "fraction of the roof NAMED IN `bound`: valu -> valu_frac (issue share x lane utilisation), hbm -> dram_frac "
                                     "(counter traffic / time / 8 TB/s), latency -> the larger of the two; `frac` (contract) stays algorithmic bytes / time / 8 TB/s",
                     "profile_avg_us": dom[1].get("profile_avg_us"), "profile_state": dom[1].get("profile_state"), "live_event_us": round(dom[1]["ms"] * 1e3, 2),
                     "counters": prof["dir"] if (prof["dir"] and dom[1].get("traffic")) else None,
                     "traffic_source": ((prof["dir"] + "/pmc_summary.json (2*FETCH_SIZE + WRITE_SIZE per launch; traffic_lo = FETCH_SIZE + WRITE_SIZE: profiles/r3_calib)"
                                         + ("" if dom[1].get("profile_state") != "stale" else " — STALE: the live kernel time is > 10 % off the profiled one")))
                                       if (prof["dir"] and dom[1].get("traffic")) else None,
                     "bound_source": (prof["dir"] + "/sq_counters.json (raw SQ_INSTS_VALU, GRBM_GUI_ACTIVE, SQ_THREAD_CYCLES_VALU, SQ_ACTIVE_INST_VALU; 1080p bench frame)") if prof["dir"] else None,
                     "algorithmic_bytes": int(dom[1]["bytes"]),
                     "note": "achieved/frac divide the ALGORITHMIC bytes (SURVEY 8d: G-buffer + mask + visited BVH nodes x 80 B + tested triangles x 48 B) by the kernel time; the node / "
                             "triangle counts are those of the TIMED kernel (occluder cache on: a ray first tests the triangle that occluded its pixel last frame), frac_full_walk uses the "
                             "counts of the cache-less walk; the ~17 MB BVH is served by L2 / Infinity Cache, so dram_frac (counter traffic) is the HBM-side figure; the operative roof of "
                             "this kernel is VALU issue: valu_frac = valu_issue_frac x lane_utilisation (= binding_frac)"},
        "stages": {n: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items()} for n, s in stages.items()},
    })
    if comm_info:
        out["comm"] = comm_info

    # ---- the other arithmetic mode, same frames, shorter run (reported, never `value`)
    other = tiling.TiledShadows(ctx, W, H, rank, world, bounds=bounds)
    other.params.exact = 1 - exact
    stage("other_mode")
    PARTIAL.update(out)
    n2 = max(20, args.steps // 4)
    el2, _ = timed_run(other, n2, 10)
    out["tolerance_mode" if exact else "exact_mode"] = {"ms_per_step": round(el2 / n2 * 1e3, 4), "value": round(total_rays / args.steps * n2 / el2 / 1e6, 2), "unit": "Mrays/s",
                                                        "steps": n2, "note": "hr_shadows_params.exact = %d on the same frames" % (1 - exact)}
    other.wait_exchange()
    torch.cuda.synchronize()
    other.pass_.close()

    # ---- the other BASELINE configurations (outside the timed region) ------------------------------------------------------------
    PARTIAL.update(out)
    if not args.no_passes and not args.obj and args.tier == "standard":
        stage("passes" if world == 1 else "hybrid_4k")
        try:
            if world == 1:
                out["passes"] = passes_block(torch, hr, HybridFrame, ctx, scene, sd, prof, exact)
                out["passes"]["hard_tier"] = hard_tier_block(torch, hr, synth, ctx, sob_d, sr_d, exact)
                try:
                    out["passes"]["instanced"] = instanced_block(torch, hr, synth, ctx, sd, sob_d, sr_d, exact)
                except Exception as e:   # a new block must not cost the line
                    out["passes"]["instanced"] = {"error": repr(e)[:200]}
            else:
                hf = HybridFrame(ctx, scene, sd, 3840, 2160, rank, world, exact=exact)
                first_cut = list(hf.bounds)
                hf.rebalance(rounds=2, barrier=barrier)     # re-cut the bands from the measured per-rank frame times (outside the timed region)
                ms = hf.time(12, 4, barrier=barrier, repeats=2)
                rays = sum(hf.ray_counts().values())
                t = torch.tensor([ms, float(rays)], dtype=torch.float64, device="cuda")
                tm = t.clone()
                dist.all_reduce(tm, op=dist.ReduceOp.MAX)
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                cm = torch.tensor([hf.shadows.time_exchange(10), hf.ao.time_exchange(10), hf.refl.time_exchange(10), hf.gi.time_allgather(10)], dtype=torch.float64, device="cuda")
                dist.all_reduce(cm, op=dist.ReduceOp.MAX)
                out["hybrid_4k"] = {"workload": "ONE 3840x2160 hybrid frame (shadows + AO 4 spp + DDGI 16x8x16x256 + half-res reflections) row-tiled over the GPUs: strong scaling (BASELINE configs[4])",
                                    "n_gpus": world, "ms_per_frame": round(float(tm[0]), 4), "frames_per_s": round(1e3 / float(tm[0]), 1),
                                    "Mrays_per_s": round(float(t[1]) / float(tm[0]) / 1e3, 1), "bands": hf.bounds, "bands_before_rebalancing": first_cut, "scaling": "strong",
                                    "comm_us_per_frame": {"shadows_exchange": round(float(cm[0]), 1), "ao_exchange": round(float(cm[1]), 1), "reflections_exchange": round(float(cm[2]), 1),
                                                          "ddgi_atlas_allgather": round(float(cm[3]), 1),
                                                          "note": "stand-alone cost of each collective (posted and waited for back to back, max over ranks); the three exchanges overlap the next "
                                                                  "frame's traces, the all-gather sits on the DDGI -> reflections chain"}}
                out["hybrid_4k"]["forked_streams"] = bool(hf.forked)
                if hf.forked_error:
                    out["hybrid_4k"]["forked_error"] = hf.forked_error
                hf.close()
        except Exception as e:   # a report next to the headline, never a reason to lose the bench line
            out["passes_error"] = repr(e)[:300]

    # ---- CPU baseline on the host cores, bounded sample, rank 0 at N=1 only -----------------------------------------------------
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        stage("cpu_baseline")
        try:
            out["cpu_baseline"] = cpu_baseline(torch, np, scene, sd, gbs, ubos, seq, sob, sr, W, H, light, synth, args)
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)[:300]}
        PARTIAL.update(out)
    stage("done")
    return out


def dump_outputs(d, torch, hr, tiled):
    """--dump-outputs: what a caller of the timed path receives after its last step — the pass's result (hr_shadows_output(HR_OUTPUT_ATROUS), RG16F,
    as float32) and its ray-trace output (the bit-packed R32_UINT visibility mask, one float64 per 32-bit word: exact); with N > 1 the rows of this
    rank's band.  ~17 MB at 1920x1080."""
    os.makedirs(d, exist_ok=True)
    denoised = tiled.band_output().float().cpu().numpy()
    mask = tiled.pass_.output(hr.OUTPUT_RAY_TRACE).cpu().numpy().view(np.uint32).astype(np.float64)
    np.save(os.path.join(d, "denoised.npy"), denoised)
    np.save(os.path.join(d, "shadow_mask.npy"), mask)


def passes_block(torch, hr, HybridFrame, ctx, scene, sd, prof, exact):
    """BASELINE configs[2], [3] and [4] on ONE GPU: wall-clock per pass and per hybrid frame, per-kernel event times and roofline fractions"""
    res = {}
    hf = HybridFrame(ctx, scene, sd, 1920, 1080, exact=exact)
    hf.time(6, 2)                                                   # warm every pass (history, atlases)
    wall = {n: hf.time(12, 4, only=n, repeats=3) for n in ("shadows", "ao", "ddgi", "reflections")}
    hybrid = hf.time(12, 4, repeats=3)
    hf.concurrent_streams(True, "streams")
    hybrid3 = hf.time(12, 6, repeats=3)
    hf.concurrent_streams(True, "graph")
    hybridg = hf.time(12, 6, repeats=3)
    hf.concurrent_streams(False)
    rays = hf.ray_counts()
    st = hf.stage_times(10)
    tb = hf.trace_bytes()
    label = {"ao": "AO 4 spp + temporal + 2 blurs, 1920x1080 (configs[2])", "reflections": "reflections 1 spp at half resolution + SVGF + upsample, 1920x1080 frame (configs[3])",
             "ddgi": "DDGI 16x8x16 probes x 256 rays: trace + probe updates + per-pixel sample, 1920x1080", "shadows": "shadows 1 spp + SVGF, 1920x1080 (inside the hybrid frame)"}
    for n in ("ao", "reflections", "ddgi", "shadows"):
        res[n] = {"workload": label[n], "ms_per_frame": round(wall[n], 4), "frames_per_s": round(1e3 / wall[n], 1), "rays_per_frame": rays[n],
                  "Mrays_per_s": round(rays[n] / wall[n] / 1e3, 1), "kernels": kernel_entries(prof, n, st[n], exact, tb.get(n))}
        res[n]["roofline"] = pass_roofline(res[n]["kernels"])
    res["hybrid_1080p"] = {"workload": "whole hybrid frame 1920x1080 on one GPU: shadows + AO 4 spp + DDGI 16x8x16x256 + half-res reflections, one stream",
                           "ms_per_frame": round(hybrid, 4), "frames_per_s": round(1e3 / hybrid, 1), "Mrays_per_s": round(sum(rays.values()) / hybrid / 1e3, 1),
                           "concurrent_streams": {"ms_per_frame": round(hybrid3, 4), "frames_per_s": round(1e3 / hybrid3, 1),
                                                  "note": "hr_hybrid_frame HR_FRAME_STREAMS (C ABI; hr::HybridFrame in include/hr/passes.hpp): shadows | AO | DDGI trace + update -> reflections | "
                                                          "DDGI sample forked over four HIP streams, joined at the end of the frame (independent chains; bit-identical images)"},
                           "hip_graph": {"ms_per_frame": round(hybridg, 4), "frames_per_s": round(1e3 / hybridg, 1),
                                         "note": "HR_FRAME_GRAPH: the same forked frame captured into one hipGraph per frame; the instantiated graph is updated in place (hipGraphExecUpdate) "
                                                 "because UBO, frame counter and ping-pong parity travel in the kernel arguments"}}
    hf.close()
    # configs[3] read as FULL-resolution reflections (the reference's default, timed above, is half resolution)
    hfr = HybridFrame(ctx, scene, sd, 1920, 1080, exact=exact, refl_scale=0)
    hfr.time(4, 2)
    ms_r = hfr.time(12, 4, only="reflections", repeats=3)
    rays_r = hfr.ray_counts()["reflections"]
    res["reflections_full_res"] = {"workload": "reflections 1 spp at FULL resolution + SVGF, 1920x1080 (configs[3] without the reference's half-resolution default)",
                                   "ms_per_frame": round(ms_r, 4), "frames_per_s": round(1e3 / ms_r, 1), "rays_per_frame": rays_r, "Mrays_per_s": round(rays_r / ms_r / 1e3, 1)}
    hfr.close()
    hf4 = HybridFrame(ctx, scene, sd, 3840, 2160, exact=exact)
    ms4 = hf4.time(8, 4, repeats=3)
    r4 = hf4.ray_counts()
    hf4.concurrent_streams(True, "streams")
    ms43 = hf4.time(8, 4, repeats=3)
    hf4.concurrent_streams(True, "graph")
    ms4g = hf4.time(8, 4, repeats=3)
    hf4.concurrent_streams(False)
    st4 = hf4.stage_times(8)
    tb4 = hf4.trace_bytes()
    prof4 = load_profile("_4k")
    res["hybrid_4k_one_gpu"] = {"workload": "whole hybrid frame 3840x2160 on ONE GPU (BASELINE configs[4] names 8)", "ms_per_frame": round(ms4, 4), "frames_per_s": round(1e3 / ms4, 1),
                                "Mrays_per_s": round(sum(r4.values()) / ms4 / 1e3, 1), "concurrent_streams": {"ms_per_frame": round(ms43, 4), "frames_per_s": round(1e3 / ms43, 1)},
                                "hip_graph": {"ms_per_frame": round(ms4g, 4), "frames_per_s": round(1e3 / ms4g, 1)},
                                "kernels": {n: kernel_entries(prof4, n, st4[n], exact, tb4.get(n)) for n in ("shadows", "ao", "ddgi", "reflections")},
                                "kernels_note": "per-kernel HIP-event times of the 4K frame; counters from " + (prof4["dir"] or "(no 4K profile committed)") +
                                                " (*_4k files: the working set of a 4K pass exceeds the 256 MiB Infinity Cache, so dram_frac is an HBM figure here)"}
    res["hybrid_4k_one_gpu"]["roofline"] = {n: pass_roofline(k) for n, k in res["hybrid_4k_one_gpu"]["kernels"].items()}
    res["hybrid_4k_one_gpu"]["roofline_note"] = ("per PASS at 3840x2160: algorithmic bytes (SURVEY 8d; trace kernels: pixels x inputs + instrumented node steps x 80 B + triangle tests x 48 B) "
                                                 "summed over the pass's kernels / summed HIP-event time / 8 TB/s; `binding` = what limits the kernel the pass spends most time in")
    hf4.close()
    res["note"] = ("kernel `frac` = algorithmic bytes (SURVEY 8d) / HIP-event time / 8 TB/s; `traffic` / `dram_frac`, `valu_issue_frac`, `lane_utilisation`, `valu_frac`, `bound` from the "
                   "rocprofv3 counters committed under " + (prof["dir"] or "profiles/ (none for this configuration)") + " by EXACT kernel instance; `profile_state` = stale when the live "
                   "event time is > 10 % off the profiled duration; the ray-trace kernels' algorithmic bytes come from their instrumented builds (hr_*_trace_stats: "
                   "node steps x 80 B + triangle tests x 48 B + the per-pixel inputs / outputs); `binding_frac` = the fraction of the roof named in `bound`")
    return res


def hard_tier_block(torch, hr, synth, ctx, sob_d, sr_d, exact):
    """the headline pass on the harder workload tier: ~2.5 M triangles, layered fabric + foliage cards, sun 20 degrees
    above the horizon — what a deep, thin-geometry BVH costs per ray"""
    W, H = 1920, 1080
    sd = synth.sponza_like(1.0, tier="hard")
    scene = hr.Scene(ctx, sd)
    light = synth.sponza_hard_light()
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(3)]
    ubos = [synth.make_ubo(cams[i + 1], cams[i], light) for i in range(2)]
    gbs = [scene.gbuffer(u, W, H) for u in ubos]
    fis = [hr.frame_inputs(gbs[k & 1], gbs[(k + 1) & 1], ubos[k & 1], k, k & 1, sob_d, sr_d) for k in range(2)]
    p = hr.RayTracedShadows(ctx, W, H)
    p.params.exact = exact
    for k in range(6):
        fis[k & 1].num_frames = k
        p.render(scene, fis[k & 1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 60
    for k in range(6, 6 + n):
        fis[k & 1].num_frames = k
        p.render(scene, fis[k & 1])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    p.set_profiling(True)
    acc = {}
    for k in range(70, 80):
        fis[k & 1].num_frames = k
        p.render(scene, fis[k & 1])
        for nme, t, b in p.stage_times():
            acc[nme] = acc.get(nme, 0.0) + t / 10
    rays = p.ray_count()
    r, nn, nt = p.trace_stats(scene, fis[0])
    out = {"workload": f"1920x1080 hard tier ({sd.n_tris} tris, {int(scene.info.n_nodes)} BVH nodes, depth {int(scene.info.max_depth)}): shadows 1 spp + SVGF",
           "ms_per_frame": round(ms, 4), "rays_per_frame": int(rays), "Mrays_per_s": round(rays / ms / 1e3, 1), "nodes_per_ray": round(nn / max(r, 1), 2),
           "tris_per_ray": round(nt / max(r, 1), 2), "trace_only_Mrays_per_s": round(rays / acc.get("ray_trace", 1e9) / 1e3, 1),
           "stage_ms": {k: round(v, 4) for k, v in acc.items()}}
    p.close(); scene.close()
    return out


def instanced_block(torch, hr, synth, ctx, sd, sob_d, sr_d, exact, movers=200, frames=30):
    """the reference's scene model (meshes + instances, the acceleration structure updated every frame: main.cpp:74): the bench building as one identity
    instance + `movers` cubes / pyramids flying through it — what hr_scene_update_instances costs per frame and what the headline pass costs on the updated
    tree against hr_scene_create over the same world vertices (masks equal)"""
    W, H = 1920, 1080
    small = synth.instanced_cornell(2)
    cube, pyr = small.meshes[1], small.meshes[2]
    lo, hi = sd.bounds()
    rng = np.random.RandomState(1)
    base = [(rng.uniform(lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo)), rng.uniform(-1, 1, 3), rng.uniform(0, 6.28), rng.uniform(6, 30, 3), rng.uniform(-2, 2, 3)) for _ in range(movers)]

    def instances(f):
        return [(synth.model_matrix(), 0, 1)] + [(synth.model_matrix(p + v * f, ax, ang + 0.05 * f, sc), 1 + (i & 1), 2 + i) for i, (p, ax, ang, sc, v) in enumerate(base)]
    isd = synth.InstancedSceneData(meshes=[sd, cube, pyr], instances=instances(0), materials=sd.materials)
    g = hr.InstancedScene(ctx, isd)
    mats = [synth.InstancedSceneData(isd.meshes, instances(f), isd.materials).matrices() for f in range(frames + 1)]
    for m in mats[:3]:
        g.update(m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for m in mats:
        g.update(m)
    torch.cuda.synchronize()
    upd_ms = (time.perf_counter() - t0) / len(mats) * 1e3
    flat = hr.Scene(ctx, isd.flatten(mats[-1]))
    cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(2)]
    ubo = synth.make_ubo(cams[1], cams[0], synth.sponza_light())
    gb = flat.gbuffer(ubo, W, H)
    fi = hr.frame_inputs(gb, gb, ubo, 0, 0, sob_d, sr_d)
    ms, masks = {}, {}
    for tag, sc in (("updated", g), ("rebuilt", flat)):
        p = hr.RayTracedShadows(ctx, W, H)
        p.params.exact = exact
        for k in range(6):
            fi.num_frames = k
            p.render(sc, fi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(6, 46):
            fi.num_frames = k
            p.render(sc, fi)
        torch.cuda.synchronize()
        ms[tag] = (time.perf_counter() - t0) / 40 * 1e3
        masks[tag] = p.image(p.IMG_MASK).clone()
        p.close()
    info = g.refresh_info()
    out = {"workload": f"bench building + {movers} moving instances ({info.n_tris} tris, {info.n_nodes} nodes), {frames} frames of motion, shadows 1 spp + SVGF at 1920x1080",
           "instances": movers + 1, "update_ms_per_frame": round(upd_ms, 4), "top_level_rebuilds": g.top_level_rebuilds,
           "ms_per_frame_updated_tree": round(ms["updated"], 4), "ms_per_frame_rebuilt_tree": round(ms["rebuilt"], 4), "masks_equal": bool(torch.equal(masks["updated"], masks["rebuilt"]))}
    g.close(); flat.close()
    return out


def cpu_baseline(torch, np, scene, sd, gbs, ubos, seq, sob, sr, W, H, light, synth, args):
    """BASELINE.md §3 / SURVEY §8d: the identical BVH (binary form) and the identical ray batch of a bench frame replayed through the
    oracle's scalar any-hit traversal (OpenMP over rays, all host threads), and the oracle's denoise chain timed on its own."""
    from oracle import pyoracle as po
    ncpu = po.set_threads()          # min(affinity, cgroup quota): the box shows 256 hardware threads and grants 16
    host = {k: {n: (t.cpu().numpy().view(np.uint16) if t.dtype == torch.float16 else t.cpu().numpy()) for n, t in gbs[k].items()} for k in seq[:3]}
    osc = po.Scene(sd)
    res = {"unit": "Mrays/s", "cores": ncpu, "kind": "port"}
    # (1) trace replay: the rays the GPU kernel fires for this frame, generated once, traversed repeatedly for ~10 s
    key = seq[1]
    rays = po.shadows_gen_rays(ubos[key], host[key]["depth"], host[key]["gb2"], sob, sr, 0.5, 1)
    rays = np.ascontiguousarray(rays[rays[:, 7] > 0.0])
    rays[:, 7] = 0.01                                                 # t_min of the shadow query (ray_query.glsl:13-27)
    _, st = osc.any_hit(rays[::16], stats=True)                       # instrumented (serial) pass on a sample: nodes / triangles per ray
    st = [float(v) * 16 for v in st]
    osc.any_hit(rays)                                                 # warm
    n_rep, t0 = 0, time.perf_counter()
    while True:
        occ = osc.any_hit(rays)
        n_rep += 1
        if time.perf_counter() - t0 > float(os.environ.get("HR_BENCH_CPU_SECONDS", "8")) or n_rep >= 400:
            break
    dt = time.perf_counter() - t0
    res["value"] = round(len(rays) * n_rep / dt / 1e6, 3)
    res["trace_replay"] = {"value": res["value"], "unit": "Mrays/s", "rays_per_batch": int(len(rays)), "batches": n_rep, "seconds": round(dt, 2),
                           "nodes_per_ray_bvh2": round(float(st[0]) / len(rays), 2), "tris_per_ray_bvh2": round(float(st[1]) / len(rays), 2),
                           "occluded_fraction": round(float(occ.mean()), 4)}
    # (1b) the same batch through the PRODUCT's tree on the host (VERDICT r4 #8 / north_star "CPU replay of the same BVH + ray batches"):
    # oracle/orc_replay8.cpp = the product's builder + the walk of csrc/traverse.h restated on the host + the oracle's triangle test
    try:
        rp = po.Replay8(sd)
        occ8, st8 = rp.any_hit(rays, stats=True)
        budget = float(os.environ.get("HR_BENCH_CPU_SECONDS", "8"))
        n8, t0 = 0, time.perf_counter()
        while True:
            occ8 = rp.any_hit(rays)
            n8 += 1
            if time.perf_counter() - t0 > budget or n8 >= 400:
                break
        dt8 = time.perf_counter() - t0
        res["trace_replay_same_tree"] = {"value": round(len(rays) * n8 / dt8 / 1e6, 3), "unit": "Mrays/s", "cores": ncpu, "batches": n8, "seconds": round(dt8, 2),
                                         "bvh_nodes": rp.num_nodes(), "nodes_per_ray": round(float(st8[0]) / len(rays), 2), "tris_per_ray": round(float(st8[1]) / len(rays), 2),
                                         "masks_equal": bool(np.array_equal(occ8, occ)),
                                         "note": "the product's 8-wide tree (csrc/bvh_build.cpp) walked on the host as csrc/traverse.h walks it on the GPU (oracle/orc_replay8.cpp)"}
    except Exception as e:
        res["trace_replay_same_tree"] = {"error": repr(e)[:200]}
    res["sample"] = (f"the {len(rays)} shadow rays of one {W}x{H} bench frame (identical origins / directions / t_max) through the oracle's scalar BVH2 any-hit "
                     f"traversal, OpenMP over rays on {ncpu} host threads (the box's cgroup CPU quota; {os.cpu_count()} hardware threads are visible), {n_rep} repetitions")
    # (2) the denoise chain of the oracle (temporal + 4 a-trous), one warm frame, for context
    op = po.ShadowsPass(W, H)
    op.render(osc, ubos[seq[0]], host[seq[0]], host[seq[0]], sob, sr, 0)
    mask, _ = po.shadows_ray_trace(osc, ubos[key], host[key]["depth"], host[key]["gb2"], sob, sr, 0.5, 1)
    t0 = time.perf_counter()
    tv, mom, tiles = po.shadows_temporal(ubos[key], mask, host[key], host[seq[0]], op.prev_image, op.moments)
    t1 = time.perf_counter()
    img = tv
    for i in range(4):
        img = po.shadows_atrous(img, host[key]["gb2"], host[key]["gb3"], tiles, 1 << i, power=1.2 if i == 3 else 0.0)
    t2 = time.perf_counter()
    res["denoise_ms"] = {"temporal": round((t1 - t0) * 1e3, 2), "atrous_x4": round((t2 - t1) * 1e3, 2), "threads": ncpu,
                         "note": "oracle restatement of shadows_denoise_reprojection.comp + 4 x shadows_denoise_atrous.comp on one 1920x1080 frame (OpenMP over rows)"}
    # (3) whole oracle frames (trace + denoise through the ctypes boundary), the figure round 1 reported
    nrays, nf = 0, max(1, args.cpu_frames)
    t0 = time.perf_counter()
    for f in range(nf):
        k1, k0 = seq[(f + 1) % 3], seq[f % 3]
        op.render(osc, ubos[k1], host[k1], host[k0], sob, sr, f + 1)
        nrays += op.stages["rays"]
    dt = time.perf_counter() - t0
    res["whole_frames"] = {"frames_per_s": round(nf / dt, 3), "Mrays_per_s": round(nrays / dt / 1e6, 3), "frames": nf}
    # (4) the reference's OWN shaders (oracle/_ref, one host thread): a small frame of the same view, trace + denoise
    try:
        from oracle import pyref, ref_harness as rh
        if pyref.available():
            rw, rhh = 240, 136
            rcams = [synth.sponza_camera(rw / rhh, frame=f, dolly=0.5) for f in range(3)]
            rubos = [synth.make_ubo(rcams[i + 1], rcams[i], light) for i in range(2)]
            rgb = [{n: (t.cpu().numpy().view(np.uint16) if t.dtype == torch.float16 else t.cpu().numpy()) for n, t in scene.gbuffer(u, rw, rhh).items()} for u in rubos]
            rp, orp = rh.RefShadowsPass(rw, rhh), po.ShadowsPass(rw, rhh)
            rp.render(osc, rubos[0], rgb[0], rgb[0], sob, sr, 0)
            orp.render(osc, rubos[0], rgb[0], rgb[0], sob, sr, 0)
            t0r = time.perf_counter()
            rp.render(osc, rubos[1], rgb[1], rgb[0], sob, sr, 1)
            dtr = time.perf_counter() - t0r
            orp.render(osc, rubos[1], rgb[1], rgb[0], sob, sr, 1)
            res["reference_shaders"] = {"value": round(orp.stages["rays"] / dtr / 1e6, 4), "unit": "Mrays/s", "cores": 1,
                                        "sample": f"one {rw}x{rhh} frame of the same view through the reference's shaders compiled for the CPU (oracle/_ref)",
                                        "bit_identical_to_port": bool(np.array_equal(rp.stages["output"], orp.stages["output"]))}
    except Exception as e:  # the baseline is a report, never a reason to lose the bench line
        res["reference_shaders"] = {"error": repr(e)[:200]}
    return res


if __name__ == "__main__":
    main()
