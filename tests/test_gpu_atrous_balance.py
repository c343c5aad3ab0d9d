"""The residency cap of kf_shadows_atrous01 and the instrumented kernels of the shadow pass's tolerance-mode a-trous chain.

kf_shadows_atrous01 (the fused a-trous iterations 0 and 1, one workgroup per 32 x 16 region) asks for unused dynamic LDS so that a CU holds at
most R of its workgroups (pass_core.h atrous_resident_pad; FT_ATROUS01_RESIDENT, or HR_ATROUS01_RESIDENT read once in hr_shadows_create).
Where a workgroup runs must not change a bit of what it writes.  A pass created with HR_ATROUS01_RESIDENT=0 launches as before and is the
reference; the settings under test are R = 3 (the largest pad a workgroup may ask for), 5, 8 (what fits anyway: the pad comes out as 0),
the shipped setting, and the shipped setting under HR_DEBUG_ATROUS_TIMELINE, which runs the instrumented kernels (the same bodies) and
must leave the same images and well-formed records behind.

Shapes, the smallest at which a launch can go wrong: 24 x 8 (one region), 40 x 24 and 72 x 40 (whole tiles), 37 x 21 (ragged: regions partly
outside the image, a last region with one tile row), 333 x 141 as the band (40, 96) with its halo (regions over the resident rows only).
Five frames with a moving camera; every shape but 24 x 8 must hold live and dead regions, a region with exactly one live tile and a
region whose liveness changes from one frame to the next, counted from the reference's tile classes."""
import contextlib
import os
import tempfile

import numpy as np
import pytest

import helpers
from hybrid_rendering_amd import synth, tiling
from test_gpu_tolerance import ATROUS_OUTLIERS, compare16, tiles_close

pytestmark = pytest.mark.gpu

# (scene, light): the two views of tests/test_gpu_atrous01_staging.py, and the atrium under a spot light, whose cone's edge gives 72 x 40 the
# region with one live tile and the region whose liveness changes that the sun leaves it without; the camera moves 1.5 units a frame
SCENES = (("cornell", "default"), ("sponza_small", "default"), ("sponza_small", "spot"))
SHAPES = [(24, 8, None), (40, 24, None), (72, 40, None), (37, 21, None), (333, 141, (40, 96))]
OFF = dict(HR_ATROUS01_RESIDENT="0")
TIMELINE = os.path.join(tempfile.gettempdir(), "hr_test_atrous_timeline_%d" % os.getpid())
SETTINGS = [dict(HR_ATROUS01_RESIDENT="3"), dict(HR_ATROUS01_RESIDENT="5"), dict(HR_ATROUS01_RESIDENT="8"),
            dict(),                                    # as shipped
            dict(HR_DEBUG_ATROUS_TIMELINE=TIMELINE)]   # ... through the instrumented kernels
VARIANTS = [dict(feedback_iteration=0), dict(feedback_iteration=1), dict(feedback_iteration=2), dict(feedback_iteration=3),
            dict(phi_normal=24.0),      # the <.., false> instantiations
            dict(reset=1)]              # reset_history() between frames 2 and 3
N_FRAMES = 5
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _remove_timeline_files():
    yield
    for kernel in ("atrous01", "atrous4", "atrous8"):
        if os.path.exists(TIMELINE + "." + kernel):
            os.remove(TIMELINE + "." + kernel)


@contextlib.contextmanager
def _env(values):
    """developer switches, read once in hr_shadows_create"""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _frames(oracle, view, W, H):
    """[(ubo, numpy G-buffer)] of five consecutive frames, made once per (view, shape) and never written to"""
    name, kind = view
    key = (view, W, H)
    if key not in _cache:
        if ("scene", name) not in _cache:
            _cache[("scene", name)] = oracle.Scene(helpers.scene_data(name))
        if name == "cornell" and (W, H) == (24, 8):
            # three tiles: from the usual place the box fills the middle one; 45 units to the right and 10 up a wall's edge crosses the first two
            base = synth.cornell_camera(W / H)
            cams = [synth.Camera(tuple(np.array(base.eye) + np.array([45.0, 10.0, 0.0]) + np.array([0.6, 0.2, -1.0]) * 1.5 * f), base.target, fov=base.fov, aspect=W / H)
                    for f in range(N_FRAMES)]
            ubos = [synth.make_ubo(cams[f], cams[f - 1] if f else None, helpers.light_for(name)) for f in range(N_FRAMES)]
            _cache[key] = [(u, _cache[("scene", name)].gbuffer(u, W, H)) for u in ubos]
        else:
            fr = helpers.make_frames(oracle, _cache[("scene", name)], name, W, H, N_FRAMES, 1.5, light_kind=kind)
            _cache[key] = [(f["ubo"], f["gb"]) for f in fr]
    return _cache[key]


def _tables():
    import torch
    if "tables" not in _cache:
        sob, sr = synth.blue_noise_tables()
        _cache["tables"] = (sob, sr, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda())
    return _cache["tables"]


def _rows(H, band):
    return (max(0, band[0] - tiling.HALO), min(H, band[1] + tiling.HALO)) if band else (0, H)


def _band(band):
    return (band[0], band[1], tiling.HALO, tiling.HISTORY_HALO) if band else None


def _inputs(hr, frames, f, sob_d, sr_d):
    return hr.frame_inputs(helpers.to_cuda(frames[f][1]), helpers.to_cuda(frames[f - 1 if f else 0][1]), frames[f][0], f, f & 1, sob_d, sr_d)


def _snapshot(hr, p, y0, y1):
    """everything the chain leaves behind, resident rows only"""
    out = {"temporal output": helpers.bits16(p.output(hr.OUTPUT_TEMPORAL_ACCUMULATION))[y0:y1],
           "a-trous output": helpers.bits16(p.output(hr.OUTPUT_ATROUS))[y0:y1],
           "a-trous image 0": helpers.bits16(p.image(p.IMG_ATROUS0))[y0:y1],
           "a-trous image 1": helpers.bits16(p.image(p.IMG_ATROUS1))[y0:y1],
           "feedback image": helpers.bits16(p.image(p.IMG_PREV))[y0:y1],
           "moments 0": helpers.bits16(p.image(p.IMG_MOMENTS0))[y0:y1],
           "moments 1": helpers.bits16(p.image(p.IMG_MOMENTS1))[y0:y1],
           "tile classes": p.image(p.IMG_TILES).cpu().numpy()[y0 // 8:(y1 + 7) // 8],
           "ray count": np.array([p.ray_count()])}
    return out


def _regions(tiles):
    """live tiles per 32 x 16 region of the resident tile rows"""
    ty, tx = tiles.shape
    gy, gx = -(-ty // 2), -(-tx // 4)
    padded = np.zeros((gy * 2, gx * 4), int)
    padded[:ty, :tx] = tiles != 0
    return padded.reshape(gy, 2, gx, 4).sum(axis=(1, 3))


def _check_records(regions, W, y0, y1, tag):
    """the three files the instrumented pass has just rewritten: every wave of every workgroup of the grid left one record, entry before exit,
    the waves of a workgroup agree, and kf_shadows_atrous01's live verdicts are the reference's live regions"""
    for kernel, rows_per_wg in (("atrous01", 16), ("atrous4", 8), ("atrous8", 8)):
        t = np.fromfile(TIMELINE + "." + kernel, dtype=np.uint64).reshape(-1, 4)
        t = t[t[:, 0] != 0]
        assert len(t) % 4 == 0 and (t[:, 1] >= t[:, 0]).all(), f"{tag} {kernel}: malformed records"
        assert set(np.unique(t[:, 3])) <= {0, 1} and (t[:, 3].reshape(-1, 4) == t[::4, 3:4]).all(), f"{tag} {kernel}: the waves of a workgroup disagree"
        assert len(t) // 4 >= -(-W // 32) * -(-(y1 - y0) // rows_per_wg), f"{tag} {kernel}: workgroups without a record"
        live = int((t[::4, 3] == 1).sum())
        if kernel == "atrous01":
            assert live == int((regions > 0).sum()), f"{tag} {kernel}: {live} live workgroups recorded, {int((regions > 0).sum())} live regions"


@pytest.mark.parametrize("params", VARIANTS, ids=lambda p: "-".join(f"{k}={v}" for k, v in p.items()))
@pytest.mark.parametrize("W,H,band", SHAPES)
def test_capped_and_instrumented_launches_leave_every_bit_where_it_was(oracle, hr, ctx, W, H, band, params):
    import torch
    sob, sr, sob_d, sr_d = _tables()
    y0, y1 = _rows(H, band)
    n_units, n_regions = -(-W // 32) * -(-(y1 - y0) // 8), -(-W // 32) * -(-(y1 - y0) // 16)
    live = dead = one_tile = changed = 0
    for view in SCENES:
        name = "%s (%s light)" % view
        frames = _frames(oracle, view, W, H)
        gsc = hr.Scene(ctx, helpers.scene_data(view[0]))
        with _env(OFF):
            ref = hr.RayTracedShadows(ctx, W, H, 0, band=_band(band))
        passes = []
        for s in SETTINGS:
            with _env(s):
                passes.append(hr.RayTracedShadows(ctx, W, H, 0, band=_band(band)))
        for g in [ref] + passes:
            g.params.exact = 0
            for k, v in params.items():
                if k != "reset":
                    setattr(g.params, k, v)
        before = None
        for f in range(N_FRAMES):
            fi = _inputs(hr, frames, f, sob_d, sr_d)
            if params.get("reset") and f == 3:
                for g in [ref] + passes:
                    g.reset_history()
            for g in [ref] + passes:
                g.render(gsc, fi)
            torch.cuda.synchronize()
            want = _snapshot(hr, ref, y0, y1)
            for s, g in zip(SETTINGS, passes):
                got = _snapshot(hr, g, y0, y1)
                for what in want:
                    assert np.array_equal(got[what], want[what]), f"{name} frame {f} {s or 'as shipped'}: {what} differs in {(got[what] != want[what]).sum()} values"
            r = _regions(want["tile classes"])
            if not params.get("phi_normal"):   # (the instrumented kernels exist for the default phi_normal)
                _check_records(r, W, y0, y1, f"{name} frame {f}")
            live, dead, one_tile = live + int((r > 0).sum()), dead + int((r == 0).sum()), one_tile + int((r == 1).sum())
            if before is not None:
                changed += int(((r > 0) != (before > 0)).sum())
            before = r
        for g in [ref] + passes:
            g.close()
        gsc.close()
    print(f"{W}x{H}: units {n_units} regions {n_regions}; over the frames: live regions {live}, dead {dead}, with one live tile {one_tile}, liveness changed {changed}")
    # (the inputs are the same in every variant; a reset_history() rewrites the history the classes come from, so the counts are asserted on the others)
    if (W, H) != (24, 8) and not params.get("reset"):
        assert n_regions > 3
        assert live > 0 and dead > 0, "the shape must hold live and dead regions"
        assert one_tile > 0, "the shape must hold a region with exactly one live tile"
        assert changed > 0, "the liveness of a region must change between two consecutive frames"


@pytest.mark.parametrize("W,H", [(40, 24), (72, 40)])
def test_whole_tile_shapes_against_the_oracle(oracle, hr, ctx, W, H):
    """a pass capped at R = 3 under the image rule of docs/TOLERANCE.md (tests/test_gpu_tolerance.py compare16: the thresholds and the counted
    allowance of the end-to-end comparison, as tests/test_gpu_atrous01_staging.py holds the same shapes)"""
    import torch
    sob, sr, sob_d, sr_d = _tables()
    for view in SCENES[:2]:
        name = view[0]
        frames = _frames(oracle, view, W, H)
        osc = _cache[("scene", name)]
        gsc = hr.Scene(ctx, helpers.scene_data(name))
        op = oracle.ShadowsPass(W, H, feedback_iteration=1)
        with _env(SETTINGS[0]):
            gp = hr.RayTracedShadows(ctx, W, H)
        gp.params.exact, gp.params.feedback_iteration = 0, 1
        for f in range(N_FRAMES):
            op.render(osc, frames[f][0], frames[f][1], frames[f - 1 if f else 0][1], sob, sr, f)
            gp.render(gsc, _inputs(hr, frames, f, sob_d, sr_d))
            torch.cuda.synchronize()
            st, tag = op.stages, f"{name} frame {f}"
            assert np.array_equal(gp.image(gp.IMG_MASK).cpu().numpy().view(np.uint32), st["mask"]), f"{tag}: mask must be bit-exact"
            ex = tiles_close(gp.image(gp.IMG_TILES).cpu().numpy(), st["tiles"], tag, shape=(H, W))
            compare16(helpers.bits16(gp.output(hr.OUTPUT_ATROUS)), st["output"], f"{tag} denoised visibility + filtered variance", exclude=ex,
                      variance_channels=(1,), outlier_pixels=ATROUS_OUTLIERS)
            compare16(helpers.bits16(gp.image(gp.IMG_PREV)), op.prev_image, f"{tag} feedback image (next frame's history)", exclude=ex,
                      variance_channels=(1,), outlier_pixels=ATROUS_OUTLIERS)
        gp.close(); gsc.close()


def test_two_frames_captured_into_a_graph_replay_like_eager_frames(oracle, hr, ctx):
    """the pad is fixed at create and nothing is allocated or decided inside a frame: two frames captured into one hipGraph and replayed
    equal the same two frames rendered eagerly by a reference pass"""
    import torch
    name, W, H = "cornell", 72, 40
    sob, sr, sob_d, sr_d = _tables()
    frames = _frames(oracle, (name, "default"), W, H)
    gsc = hr.Scene(ctx, helpers.scene_data(name))
    with _env(OFF):
        eager = hr.RayTracedShadows(ctx, W, H)
    with _env(SETTINGS[1]):
        graphed = hr.RayTracedShadows(ctx, W, H)
    fis = [_inputs(hr, frames, f, sob_d, sr_d) for f in range(3)]
    for p in (eager, graphed):
        p.params.exact = 0
        p.render(gsc, fis[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.render(gsc, fis[1])
        graphed.render(gsc, fis[2])
    g.replay()
    eager.render(gsc, fis[1])
    eager.render(gsc, fis[2])
    torch.cuda.synchronize()
    want, got = _snapshot(hr, eager, 0, H), _snapshot(hr, graphed, 0, H)
    for what in want:
        assert np.array_equal(got[what], want[what]), f"{what} of the replayed frames differs in {(got[what] != want[what]).sum()} values"
    eager.close(); graphed.close(); gsc.close()
