"""k_ddgi_probe_update (both instantiations: depth_sharpness 50, the written-out power, and 37, the generic one) on the crafted ray images of
tests/closest_cases.py — no tracing: radiance and direction / distance are injected through the pass's writable views, the previous atlases
through current_read(), a sentinel through current_write().  What a scene's rays reach only by luck: fp16 SUBNORMAL directions whose dot
product with a texel's direction sits just over and just under the 1e-8 threshold (irradiance), short directions whose dot product to the
50th / 37th power does (depth), probes with ONE live ray at the last slot of an LDS batch or of the four-ray unroll's tail, probes whose rays
are all skipped, distances 0 / -0 / negative / the miss value 10000 / max_distance + 0.01 +- fp16 ulps, ray counts 1, 3, 255, 256, 257, 513,
depth sides 2, 8, 9, 11, 12, 16 (the irradiance threads start at 64 / 128 / 192 / 256), irradiance sides 2, 7, 8, 16, hysteresis 0 / 1 / 0.98,
the first and a later frame, a shard with gy0 > 0.

Reference: orc_ddgi_probe_update + orc_ddgi_border_update over sentinel-filled atlases, bit for bit, EVERY texel (the outer frame and the
slabs outside a shard must keep the sentinel); the borders also against the copy rule written down in closest_cases.expect_borders; the
hysteresis-1 case also against the previous atlas itself.  tests/test_closest_cases.py keeps this from passing vacuously.
Mutation results: docs/EXPERIMENTS.md, "Adversarial inputs for the closest-hit launches and the probe update"."""
import numpy as np
import pytest

import closest_cases as cc
import helpers
from test_gpu_nonfinite import _put

pytestmark = pytest.mark.gpu


def describe(case, depth_probe, y, x):
    """the probe, family and texel of atlas position (y, x), and the rays aimed at that texel, in hex"""
    d = case["ddgi"]
    side = int(d["depth_probe_side_length" if depth_probe else "irradiance_probe_side_length"])
    per_row = int(d["probe_counts"][0]) * int(d["probe_counts"][1])
    gx, gy = (x - 1) // (side + 2), (y - 1) // (side + 2)
    if not (0 <= gx < per_row and 0 <= gy < int(d["probe_counts"][2])) or x < 1 or y < 1:
        return f"texel ({x}, {y}): the atlas' outer frame"
    probe, lx, ly = gx + per_row * gy, (x - 1) % (side + 2) - 1, (y - 1) % (side + 2) - 1
    s = f"texel ({x}, {y}) = probe {probe} [{cc.UPDATE_FAMILIES[case['family'][probe]]}] cell ({lx}, {ly})"
    if 0 <= lx < side and 0 <= ly < side:
        a = case["aimed"][probe]
        rays = np.flatnonzero((a[:, 0] == int(depth_probe)) & (a[:, 1] == ly * side + lx))[:4]
        s += "".join(f"; ray {r} ({'taken' if a[r, 2] == 0 else 'skipped'}) d = {' '.join(float(v).hex() for v in case['dirs'][probe, r])}" for r in rays)
    else:
        s += " (border)"
    return s


def assert_atlas(case, depth_probe, got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    print(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} texels differ")
    assert len(bad) == 0, f"{what}: {len(bad)} texels differ\n" + "\n".join(
        f"  {describe(case, depth_probe, int(y), int(x))}: got {[hex(int(v)) for v in got[y, x]]} want {[hex(int(v)) for v in want[y, x]]}" for y, x in bad[:8])


@pytest.mark.parametrize("case", cc.update_cases(), ids=lambda c: c["name"])
def test_probe_update_matches_the_oracle_on_every_texel(oracle, hr, ctx, case):
    import torch
    from hybrid_rendering_amd import api_gi
    d = case["ddgi"]
    counts = tuple(int(v) for v in d["probe_counts"])
    gp = api_gi.DDGI(ctx, 16, 16, d)
    try:
        if not case["first"]:
            gp.end_frame()          # a later frame: first_frame off, the atlases swapped
        _put(gp.image(gp.IMG_RADIANCE), case["rad"])
        _put(gp.image(gp.IMG_DIRDIST), case["dd"])
        ri, rd = gp.current_read()
        _put(ri, case["prev_irr"])
        _put(rd, case["prev_dep"])
        wi, wd = gp.current_write()
        _put(wi, np.full_like(case["prev_irr"], cc.SENTINEL))
        _put(wd, np.full_like(case["prev_dep"], cc.SENTINEL))
        if case["shard"] is not None:
            gp.set_shard(case["shard"][0], case["shard"][1], 0, 16)
        gp.probe_update()
        torch.cuda.synchronize()
        got_i, got_d = helpers.bits16(wi).reshape(case["prev_irr"].shape), helpers.bits16(wd).reshape(case["prev_dep"].shape)
        assert np.array_equal(helpers.bits16(ri).reshape(case["prev_irr"].shape), case["prev_irr"]), "the probe update wrote the atlas it reads"
    finally:
        gp.close()
    ref_i, ref_d = cc.update_reference(case)
    assert_atlas(case, False, got_i, ref_i, f"{case['name']}: irradiance atlas")
    assert_atlas(case, True, got_d, ref_d, f"{case['name']}: depth atlas")
    # independent of the oracle: the borders by the copy rule over the kernel's own interior; with hysteresis 1 the interior IS the previous one
    z0, z1 = case["shard"] if case["shard"] is not None else (0, counts[2])
    for depth_probe, got, prev in ((False, got_i, case["prev_irr"]), (True, got_d, case["prev_dep"])):
        side = int(d["depth_probe_side_length" if depth_probe else "irradiance_probe_side_length"])
        rows = cc.cell_rows(side, z0, z1)
        assert_atlas(case, depth_probe, got[rows], cc.expect_borders(got, side, counts)[rows], f"{case['name']}: {'depth' if depth_probe else 'irradiance'} borders by the copy rule")
        if float(d["hysteresis"]) == 1.0 and not case["first"]:
            c = 2 if depth_probe else 3
            for probe in range(z0 * counts[0] * counts[1], z1 * counts[0] * counts[1]):
                assert np.array_equal(cc.interior(got, side, counts, probe)[..., :c], cc.interior(prev, side, counts, probe)[..., :c]), (case["name"], probe, "hysteresis 1 keeps the history")
