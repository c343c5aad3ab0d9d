"""The paired history loads of kf_shadows_temporal (csrc/pass_args.h TemporalPaths, Reproj::issue) against the loads they replaced.

On the record path the first run of the pixel program fetches the two taps of a footprint row with one load per image (TP_PAIRS) instead
of one load per tap and image.  The developer switch HR_TEMPORAL_PAIRS=0, which hr_shadows_create reads once, selects the instantiation
with the older loads.  The pair is a re-statement of which bytes are loaded, not of what is computed from them, so a pass with the pairs
and a pass without must agree BIT FOR BIT on every image the temporal stage writes (temporal output, moments, geometry records of both
slots — the slots alternate frame by frame —, tile classes), on what the a-trous chain makes of them, and on the ray count; four frames
with a moving camera, so that the record path, history taps on both sides of every image edge and the feedback loop all run.  (The test
was written for five forms of the hot path, docs/EXPERIMENTS.md "Shadow temporal kernel"; SWITCHES lists the ones that are left, and the
passes are: all on, each one off, all off.)

The frames are a Cornell box seen from outside and off-centre, so that every shape holds tiles that are all sky, tiles that mix sky and
geometry and tiles of geometry only — pixels whose history footprint crosses into sky, out of the image on the left, and into rows a band
does not hold; this is asserted.  Threads without a pixel ("edge" lanes, which reproject and vote like the unguarded shader threads) exist
where the extent is no multiple of 8: 333 x 141 and 37 x 21; 40 x 24 and 72 x 40 are whole tiles, their image-edge tiles exercise the
history taps that leave the image.  333 x 141 runs as the row band (40, 96) with its halo, the smaller shapes as whole frames.

One case per small shape also holds the default pass to the oracle under the rule of docs/TOLERANCE.md (the runners of
tests/test_gpu_tolerance.py)."""
import os

import numpy as np
import pytest

import helpers
from hybrid_rendering_amd import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("HR_TEMPORAL_PAIRS",)
N_FRAMES = 4
HALO, HISTORY_HALO = 24, 40


def _cameras(aspect, n):
    return [synth.Camera((50.0 + 6.0 * f, 52.0 + 2.0 * f, 300.0 - 5.0 * f), (95.0, 42.0, 0.0), fov=40.0, aspect=aspect) for f in range(n)]


def _ubos(W, H):
    cams, light = _cameras(W / H, N_FRAMES + 1), synth.cornell_light(hard=False)
    return [synth.make_ubo(cams[f + 1], cams[f], light) for f in range(N_FRAMES)]


def _created_with(off, make):
    """make() under the switches `off` set to 0 (they are read once, in hr_shadows_create)"""
    for k in off:
        os.environ[k] = "0"
    try:
        return make()
    finally:
        for k in off:
            del os.environ[k]


def _tile_kinds(depth, y0, y1):
    """(all sky, sky and geometry, geometry only, holds threads without a pixel) tile counts over the resident rows [y0, y1)"""
    h, w = depth.shape
    ty, tx = (h + 7) // 8, (w + 7) // 8
    sky, inside = np.zeros((ty * 8, tx * 8), bool), np.zeros((ty * 8, tx * 8), bool)
    sky[:h, :w] = depth == 1.0
    inside[:h, :w] = True
    tiles = lambda a: a.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)[y0 // 8:(y1 + 7) // 8]
    s, i = tiles(sky), tiles(inside)
    return (int((s & i).all(-1).sum()), int(((s & i).any(-1) & (~s & i).any(-1)).sum()), int(((~s & i).all(-1)).sum()), int((~i.all(-1)).sum()))


def _np(t):
    import torch
    return helpers.bits16(t) if t.dtype == torch.float16 else t.cpu().numpy()


@pytest.mark.parametrize("W,H,band", [(40, 24, None), (72, 40, None), (37, 21, None), (333, 141, (40, 96))])
def test_every_path_writes_the_bits_of_the_form_it_replaced(hr, ctx, W, H, band):
    import torch
    gsc = hr.Scene(ctx, synth.cornell32())
    ubos = _ubos(W, H)
    gbs = [gsc.gbuffer(u, W, H) for u in ubos]
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    y0, y1 = (max(band[0] - HALO, 0), min(band[1] + HALO, H)) if band else (0, H)
    make = lambda: hr.RayTracedShadows(ctx, W, H, 0, band=(band[0], band[1], HALO, HISTORY_HALO) if band else None)
    passes = {"all on": make()}
    for k in SWITCHES:
        passes[k + "=0"] = _created_with((k,), make)
    passes["all off"] = _created_with(SWITCHES, make)
    for p in passes.values():
        p.params.exact = 0
    ref = passes["all on"]
    for f in range(N_FRAMES):
        n_sky, n_mixed, n_geo, n_ragged = _tile_kinds(gbs[f]["depth"].cpu().numpy(), y0, y1)
        assert n_sky > 0 and n_mixed > 0 and n_geo > 0, f"frame {f}: {n_sky} all-sky, {n_mixed} mixed, {n_geo} geometry-only tiles: a path would be tested vacuously"
        assert (n_ragged > 0) == (W % 8 != 0 or (H % 8 != 0 and y1 == H)), (f, n_ragged)
        fi = hr.frame_inputs(gbs[f], gbs[f - 1] if f else gbs[f], ubos[f], f, f & 1, sob_d, sr_d)
        for p in passes.values():
            p.render(gsc, fi)
        torch.cuda.synchronize()
        images = lambda p: [("temporal output", p.image(p.IMG_TEMPORAL)), ("moments", p.image(p.IMG_MOMENTS1 if f & 1 else p.IMG_MOMENTS0)),
                            ("geometry records (slot %d)" % (f & 1), p.image(p.IMG_GEO)), ("a-trous output", p.output(hr.OUTPUT_ATROUS)), ("feedback image", p.image(p.IMG_PREV))]
        want, want_tiles, want_rays = [(n, _np(t)) for n, t in images(ref)], ref.image(ref.IMG_TILES).cpu().numpy(), ref.ray_count()
        assert want_rays > 0 and want_tiles[y0 // 8:(y1 + 7) // 8].any() and not want_tiles[y0 // 8:(y1 + 7) // 8].all(), f"frame {f}: every tile has one class"
        for name, p in passes.items():
            if p is ref:
                continue
            for (label, a), (_, t) in zip(want, images(p)):
                b = _np(t)
                assert a.shape == b.shape and a.shape[0] == H, (label, a.shape, b.shape)
                assert np.array_equal(a[y0:y1], b[y0:y1]), f"{name}, frame {f}: {label} differs in {(a[y0:y1] != b[y0:y1]).sum()} values"
            got_tiles = p.image(p.IMG_TILES).cpu().numpy()
            assert np.array_equal(want_tiles[y0 // 8:(y1 + 7) // 8], got_tiles[y0 // 8:(y1 + 7) // 8]), f"{name}, frame {f}: tile classes differ"
            assert p.ray_count() == want_rays, f"{name}, frame {f}: ray count"
    for p in passes.values():
        p.close()
    gsc.close()


@pytest.mark.parametrize("W,H", [(40, 24), (72, 40), (37, 21)])
def test_all_paths_on_against_the_oracle(oracle, hr, ctx, W, H):
    import torch
    import test_gpu_tolerance as tol
    sd = synth.cornell32()
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
    ubos = _ubos(W, H)
    gbs = [osc.gbuffer(u, W, H) for u in ubos]
    sob, sr = synth.blue_noise_tables()
    sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
    gp, op = hr.RayTracedShadows(ctx, W, H), oracle.ShadowsPass(W, H)
    gp.params.exact = 0
    dev = [helpers.to_cuda(g) for g in gbs]
    for f in range(N_FRAMES):
        cur, prev = gbs[f], gbs[f - 1 if f else 0]
        op.render(osc, ubos[f], cur, prev, sob, sr, f)
        gp.render(gsc, hr.frame_inputs(dev[f], dev[f - 1 if f else 0], ubos[f], f, f & 1, sob_d, sr_d))
        torch.cuda.synchronize()
        st = op.stages
        assert np.array_equal(gp.image(gp.IMG_MASK).cpu().numpy().view(np.uint32), st["mask"]), f"frame {f}: mask must be bit-exact"
        assert gp.ray_count() == st["rays"]
        ex = tol.tiles_close(gp.image(gp.IMG_TILES).cpu().numpy(), st["tiles"], f"frame {f}", shape=(H, W))
        tol.compare16(helpers.bits16(gp.image(gp.IMG_TEMPORAL)), st["temporal"], f"frame {f} temporal", abs_floor=tol.INTERMEDIATE_FLOOR)
        tol.compare16(helpers.bits16(gp.image(gp.IMG_MOMENTS1 if f & 1 else gp.IMG_MOMENTS0)), st["moments"], f"frame {f} moments", abs_floor=tol.INTERMEDIATE_FLOOR)
        tol.compare16(helpers.bits16(gp.output(hr.OUTPUT_ATROUS)), st["output"], f"frame {f} denoised visibility + filtered variance", exclude=ex, variance_channels=(1,),
                      outlier_pixels=tol.ATROUS_OUTLIERS)
        tol.compare16(helpers.bits16(gp.image(gp.IMG_PREV)), op.prev_image, f"frame {f} feedback image", exclude=ex, variance_channels=(1,), outlier_pixels=tol.ATROUS_OUTLIERS)
    gp.close(); gsc.close()
