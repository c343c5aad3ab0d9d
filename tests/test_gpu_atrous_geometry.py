"""The tolerance-mode shadow a-trous gather kernel after its fetches were reordered.

kf_shadows_atrous<4 | 8> fetches the classes of its four tiles as the aligned dwords that hold them (a wave-uniform load) and requests
every texel of a pixel — centre, 3x3 variance, 8 taps — in one batch, testing the centre for sky afterwards.  The shapes are the
smallest at which that can go wrong:

  * 40 x 24      tiles_x = 5 (the second workgroup column covers one tile: its class dwords run into the next tile row and, in the
                 last row, past the last tile), a partial workgroup column, taps at distance 8 leave the image on both sides
  * 72 x 40      tiles_x = 9: the class dword of a workgroup is misaligned in every tile row
  * 333 x 141    rows (40, 96) as a band plus the tiling halos: resident rows that are not the image's

Every shape holds sky pixels inside filtered tiles and copied (class 0) tiles next to filtered ones — asserted below from IMG_TILES
and the depth image, so a change of the scenes cannot hollow the cases out.
"""
import numpy as np
import pytest

import helpers
from hybrid_rendering_amd import synth, tiling
from test_gpu_tolerance import ATROUS_OUTLIERS, compare16, tiles_close

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "sponza_small")
SHAPES = [(40, 24, None), (72, 40, None), (333, 141, (40, 96))]
N_FRAMES = 4
_cache = {}


def _frames(oracle, name, W, H):
    """[(ubo, numpy G-buffer)] of four consecutive frames, made once per (scene, shape) and never written to"""
    key = (name, W, H)
    if key not in _cache:
        if ("scene", name) not in _cache:
            _cache[("scene", name)] = oracle.Scene(helpers.scene_data(name))
        fr = helpers.make_frames(oracle, _cache[("scene", name)], name, W, H, N_FRAMES, 1.5)
        _cache[key] = [(f["ubo"], f["gb"]) for f in fr]
    return _cache[key]


def _tables():
    import torch
    sob, sr = synth.blue_noise_tables()
    return sob, sr, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()


def _rows(H, band):
    """every resident row: the band and its halo"""
    return (max(0, band[0] - tiling.HALO), min(H, band[1] + tiling.HALO)) if band else (0, H)


def _band(band):
    return (band[0], band[1], tiling.HALO, tiling.HISTORY_HALO) if band else None


def _inputs(hr, frames, f, sob_d, sr_d):
    return hr.frame_inputs(helpers.to_cuda(frames[f][1]), helpers.to_cuda(frames[f - 1 if f else 0][1]), frames[f][0], f, f & 1, sob_d, sr_d)


def _scene_checks(tiles, depth, y0, y1):
    """(sky pixels inside class-1 tiles, class-0 tiles next to class-1 tiles) over the resident rows"""
    t = tiles.astype(bool)
    H, W = depth.shape
    live = np.kron(t, np.ones((8, 8), bool))[:H, :W]
    p = np.pad(t, 1)
    near = p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return int(((depth == 1.0) & live)[y0:y1].sum()), int((~t & near)[y0 // 8:(y1 + 7) // 8].sum())


@pytest.mark.parametrize("W,H,band,params", [(w, h, b, None) for w, h, b in SHAPES] + [
    (72, 40, None, dict(filter_iterations=2, power=2.0)),
    (40, 24, None, dict(feedback_iteration=0)),
    # the feedback image written by the gather kernel itself (its second store, in the copied-tile branch and in the pixel function)
    (40, 24, None, dict(feedback_iteration=2)),
    (72, 40, None, dict(feedback_iteration=3)),
    (333, 141, (40, 96), dict(feedback_iteration=2)),
])
def test_the_two_kernel_sets_agree_bit_for_bit(oracle, hr, ctx, W, H, band, params):
    """render() (kf_shadows_atrous01, then kf_shadows_atrous<4>, <8>) against the stage entry points of a pass created with HR_FUSE=0
    (kf_shadows_atrous_lds<1>, <2>, then <4>, <8>): a-trous output and feedback image, every resident row, every frame.  The two sets
    clamp and zero-fill by different code, and what the gather kernel reads at distance 4 and 8 is what they wrote."""
    import os
    import torch
    sob, sr, sob_d, sr_d = _tables()
    y0, y1 = _rows(H, band)
    sky_live = mixed = 0
    for name in SCENES:
        frames = _frames(oracle, name, W, H)
        gsc = hr.Scene(ctx, helpers.scene_data(name))
        fused = hr.RayTracedShadows(ctx, W, H, 0, band=_band(band))
        os.environ["HR_FUSE"] = "0"   # developer switch, read once in hr_shadows_create
        try:
            staged = hr.RayTracedShadows(ctx, W, H, 0, band=_band(band))
        finally:
            del os.environ["HR_FUSE"]
        for g in (fused, staged):
            g.params.exact = 0
            for k, v in (params or {}).items():
                setattr(g.params, k, v)
        for f in range(N_FRAMES):
            fi = _inputs(hr, frames, f, sob_d, sr_d)
            fused.render(gsc, fi)
            staged.ray_trace(gsc, fi)
            staged.temporal(fi)
            for i in range(int(staged.params.filter_iterations)):
                staged.atrous_iteration(fi, i)
            torch.cuda.synchronize()
            for what, a, b in (("a-trous output", fused.output(hr.OUTPUT_ATROUS), staged.output(hr.OUTPUT_ATROUS)),
                               ("feedback image", fused.image(fused.IMG_PREV), staged.image(staged.IMG_PREV))):
                a, b = helpers.bits16(a)[y0:y1], helpers.bits16(b)[y0:y1]
                assert np.array_equal(a, b), f"{name} frame {f}: {what} of the two kernel sets differs in {(a != b).sum()} halfs"
            fb = (params or {}).get("feedback_iteration", 1)
            if fb >= 2:   # the gather kernel's second store: the feedback image is the image that iteration wrote (IMG_ATROUS1 for 2, IMG_ATROUS0 for 3)
                a, b = helpers.bits16(fused.image(fused.IMG_PREV))[y0:y1], helpers.bits16(fused.image(fused.IMG_ATROUS0 if fb & 1 else fused.IMG_ATROUS1))[y0:y1]
                assert np.array_equal(a, b), f"{name} frame {f}: the feedback copy of iteration {fb} differs from its output in {(a != b).sum()} halfs"
            tiles = fused.image(fused.IMG_TILES).cpu().numpy()
            assert np.array_equal(tiles[y0 // 8:(y1 + 7) // 8], staged.image(staged.IMG_TILES).cpu().numpy()[y0 // 8:(y1 + 7) // 8])
            s, m = _scene_checks(tiles, frames[f][1]["depth"], y0, y1)
            sky_live, mixed = sky_live + s, mixed + m
        fused.close(); staged.close(); gsc.close()
    assert sky_live > 0, "the shape must hold sky pixels inside filtered tiles (the centre test the gather kernel applies after its loads)"
    assert mixed > 0, "the shape must hold copied tiles next to filtered ones (the class fetches)"


@pytest.mark.parametrize("W,H,feedback", [(40, 24, 1), (72, 40, 1), (72, 40, 2)])
def test_small_shapes_against_the_oracle(oracle, hr, ctx, W, H, feedback):
    """the denoised image and the feedback image under the image rule of docs/TOLERANCE.md (tests/test_gpu_tolerance.py compare16: the
    thresholds and the counted allowance of test_shadows_tolerance's end-to-end comparison, nothing new)"""
    import torch
    sob, sr, sob_d, sr_d = _tables()
    for name in SCENES:
        frames = _frames(oracle, name, W, H)
        osc = _cache[("scene", name)]
        gsc = hr.Scene(ctx, helpers.scene_data(name))
        gp, op = hr.RayTracedShadows(ctx, W, H), oracle.ShadowsPass(W, H, feedback_iteration=feedback)
        gp.params.exact, gp.params.feedback_iteration = 0, feedback
        for f in range(N_FRAMES):
            cur, prev = frames[f][1], frames[f - 1 if f else 0][1]
            op.render(osc, frames[f][0], cur, prev, sob, sr, f)
            gp.render(gsc, _inputs(hr, frames, f, sob_d, sr_d))
            torch.cuda.synchronize()
            st = op.stages
            assert np.array_equal(gp.image(gp.IMG_MASK).cpu().numpy().view(np.uint32), st["mask"]), f"{name} frame {f}: mask must be bit-exact"
            ex = tiles_close(gp.image(gp.IMG_TILES).cpu().numpy(), st["tiles"], f"{name} frame {f}", shape=(H, W))
            compare16(helpers.bits16(gp.output(hr.OUTPUT_ATROUS)), st["output"], f"{name} frame {f} denoised visibility + filtered variance", exclude=ex,
                      variance_channels=(1,), outlier_pixels=ATROUS_OUTLIERS)
            compare16(helpers.bits16(gp.image(gp.IMG_PREV)), op.prev_image, f"{name} frame {f} feedback image (next frame's history)", exclude=ex,
                      variance_channels=(1,), outlier_pixels=ATROUS_OUTLIERS)
        gp.close(); gsc.close()
