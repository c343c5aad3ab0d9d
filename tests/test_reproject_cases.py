"""tests/reproject_cases.py checks itself (numpy), shows with the ORACLE ALONE that its plane-distance and normal ladders straddle their
thresholds, and pins the oracle to the reference's own shaders on the crafted sequences — the quirk branches of reprojection.glsl (negative
coordinates, zero reads outside the image, the 3x3 fallback at a border) that rendered frames hardly reach."""
import numpy as np
import pytest

import helpers
import reproject_cases as rc
from hybrid_rendering_amd import synth, synth_env
from oracle import pyref

CASES = [(n, w, h) for n in rc.SCENES for (w, h) in rc.SIZES]


@pytest.mark.parametrize("name,w,h", CASES)
def test_generator(oracle, name, w, h):
    osc, frames, info = rc.sequence(oracle, name, w, h)
    H, C = frames[rc.FRAME_H]["gb"], frames[rc.FRAME_C]["gb"]
    fam = info["family"]
    for f, v in rc.FAMILY.items():
        assert (fam == v).any(), f"family {f} is missing at {w}x{h}"
    starts = [r0 for r0, _ in info["rows"].values()]
    assert all(r % 8 for r in starts), f"a stripe starts on a tile row: {info['rows']}"
    # valid G-buffers: finite, |mv| <= 2 extents, integer mesh ids <= 2048
    for G in (H, C):
        mv, ids = rc.f16val(G["gb2"][..., 2:]), rc.f16val(G["gb3"][..., 2])
        assert np.isfinite(mv).all() and np.abs(mv).max() <= 2.0
        assert np.isfinite(G["depth"]).all() and (G["depth"] >= 0).all() and (G["depth"] <= 1).all()
        assert (ids == np.round(ids)).all() and ids.min() >= 0 and ids.max() <= 2048
        assert all(np.isfinite(rc.f16val(G[k])).all() for k in ("gb2", "gb3"))
    # A: every listed position is reached on both axes — exactly where an fp16 motion vector can, else in the same zone of every decision
    A = info["A"]
    for axis, ext, key in ((0, w, "hfx"), (1, h, "hfy")):
        for i, t in enumerate(rc.targets(ext)):
            got = A[(A["axis"] == axis) & (A["target"] == i)][key]
            assert len(got), (axis, float(t))
            # the recorded coordinate is what the kernel computes from the stored motion vector
            err = np.abs(got.astype(np.float64) - float(t)).min()
            print(f"A {w}x{h} axis {axis} target {float(t)!r}: nearest obtained {float(got[np.argmin(np.abs(got - t))])!r} (|diff| {err:.3e})")
            same = (rc.zone(got) == rc.zone(t)).all(-1)
            cand = np.arange(w) if axis == 0 else np.concatenate([np.arange(*info["rows"][k]) for k in ("A", "A2")])   # where family A may put the pixel
            exact_possible = (rc.aim(cand, t, ext)[1] == t).any()
            zone_possible = (rc.zone(rc.aim(cand, t, ext)[1]) == rc.zone(t)).all(-1).any()
            # exactly where some pixel's fp16 motion vector reaches the position; else in its zone of every decision where one reaches that; only
            # where no fp16 motion vector from any allowed pixel lands in the zone, the nearest obtainable coordinate within 2^-6
            assert (got == t).any() if exact_possible else same.any() if zone_possible else err <= 2.0 ** -6, (axis, float(t), got.tolist())
    for r in A:        # the stored words give the recorded coordinates
        assert rc.hist_coord(r["x"], C["gb2"][r["y"], r["x"], 2], w) == r["hfx"] and rc.hist_coord(r["y"], C["gb2"][r["y"], r["x"], 3], h) == r["hfy"]
    assert (A["axis"] == 2).sum() == 16
    # B: interior cells of all 28 patterns, and cells at each border
    pats = rc.cell_patterns()
    assert len({c // 10 for c in info["B"]["case"] if c < 1000}) == len(pats) == 28
    for p, pool in enumerate(rc.POOLS):     # every pattern that stays distinct once its outside texels cannot match, at every border, under every shift
        distinct = len({(m & rc.cell_inside(pool)).tobytes() for _, m in pats})
        placed = {c % 1000 // 10 for c in info["B"]["case"] if c // 1000 == p}
        assert len(placed) == distinct, f"B {pool} at {w}x{h}: {len(placed)} of {distinct} distinct patterns placed (a pool of cells ran dry)"
        for ci in placed:
            assert {c % 10 for c in info["B"]["case"] if c // 10 == 100 * p + ci} == set(range(len(rc.SHIFTS))), (pool, ci)
    # F: all 8 sky cells (far / wall depth x sky under all, one, two, one taps), each under 3 shifts twice, and 24 sky current pixels
    Fs = info["F"]
    assert len({c // 100 for c in Fs["case"][Fs["kind"] < 2]}) == 8 and (Fs["kind"] < 2).sum() == 8 * 3 * 2 and (Fs["kind"] == 2).sum() == 24, f"F at {w}x{h}"
    assert {(int(k), int(s)) for k, s in zip(Fs["kind"], Fs["sky_taps"]) if k < 2} == {(k, s) for k in (0, 1) for s in (15, 1, 6, 8)}
    # C: 64 on each side, distances reported
    Cc = info["C"]
    assert (Cc["ulps"] < 0).sum() == 64 and (Cc["ulps"] >= 0).sum() == 64
    for r in Cc:
        fx, fy = (rc.hist_coord(r["x"], C["gb2"][r["y"], r["x"], 2], w), rc.hist_coord(r["y"], C["gb2"][r["y"], r["x"], 3], h))
        assert rc.sumw32(fx - np.floor(fx), fy - np.floor(fy), int(r["subset"])) == r["sumw"]
        # the intended subset IS the set of footprint taps that carry the pixel's mesh id in frame H (all of them wall texels: the id alone decides).
        # The oracle's stage images cannot show this verdict: below 0.01 the 3x3 fallback accepts the same texels and the stored length is the same
        bx, by = int(np.floor(fx)), int(np.floor(fy))
        ids = [H["gb3"][by + (k >> 1), bx + (k & 1), 2] == C["gb3"][r["y"], r["x"], 2] for k in range(4)]
        assert sum(int(m) << k for k, m in enumerate(ids)) == r["subset"], (r, ids)
        assert all(H["depth"][by + (k >> 1), bx + (k & 1)] == np.float32(info["d0"]) for k in range(4))
    below, above = Cc["ulps"][Cc["ulps"] < 0], Cc["ulps"][Cc["ulps"] >= 0]
    print(f"C {name} {w}x{h}: sumw from below: closest {below.max()} ulp, 64th {below.min()} ulp; from above: closest {above.min()} ulp, 64th {above.max()} ulp of 0.01f")
    for f in "DE":
        assert (info[f]["sparse"] == 0).sum() >= 64 and (info[f]["sparse"] == 1).sum() >= 16, f
    assert set(info["D"]["ulp"]) == set(rc.LADDER.tolist())
    assert np.abs(info["E"]["dist"]).max() <= 1e-5 and (info["E"]["dist"] > 0).any() and (info["E"]["dist"] < 0).any()


def _oracle_verdicts(oracle, name, w, h):
    osc, frames, info = rc.sequence(oracle, name, w, h)
    sob, sr = synth.blue_noise_tables()
    sp, ap = oracle.ShadowsPass(w, h), oracle.AOPass(w, h, spp=2, zbp=synth.z_buffer_params())
    for f in range(rc.FRAME_C + 1):
        cur, prev = frames[f]["gb"], frames[f - 1 if f else 0]["gb"]
        sp.render(osc, frames[f]["ubo"], cur, prev, sob, sr, f)
        ap.render(osc, frames[f]["ubo"], cur, prev, sob, sr, f)
    return info, rc.reset_set(sp.stages["moments"][..., 2]), rc.reset_set(ap.stages["length"])


@pytest.mark.parametrize("name,w,h", CASES)
def test_ladders_straddle_their_thresholds(oracle, name, w, h):
    """D and E with the oracle alone: in each of D-dense, D-sparse, E-dense, E-sparse at least a quarter of the pixels is accepted and at least
    a quarter rejected (if not, the generator is wrong, not a kernel)"""
    info, s_reset, a_reset = _oracle_verdicts(oracle, name, w, h)
    assert np.array_equal(s_reset[info["family"] >= 4], a_reset[info["family"] >= 4])   # one reprojection, two passes
    for f in "DE":
        for lay, what in enumerate(("dense", "sparse")):
            r = info[f][info[f]["sparse"] == lay]
            rej = s_reset[r["y"], r["x"]]
            print(f"{f}-{what} {name} {w}x{h}: {len(r)} pixels, {rej.mean() * 100:.1f} % rejected")
            if f == "D":
                acc_ulps = sorted(set(r["ulp"][~rej].tolist())); rej_ulps = sorted(set(r["ulp"][rej].tolist()))
                print(f"   offsets accepted somewhere: {acc_ulps[:3]} .. {acc_ulps[-3:]}, rejected somewhere: {rej_ulps[:3]} .. {rej_ulps[-3:]}")
            assert 0.25 <= rej.mean() <= 0.75, (f, what, float(rej.mean()))


@pytest.mark.skipif(not pyref.available(), reason="neither /root/reference nor a prebuilt oracle/_ref")
@pytest.mark.parametrize("name,w,h", CASES)
def test_oracle_equals_the_reference_shaders(oracle, name, w, h):
    """every stage image of every frame, shadows / AO / reflections, bit for bit"""
    from oracle import ref_harness as rh, pyoracle_ddgi as od, pyoracle_reflections as orf
    osc, frames, info = rc.sequence(oracle, name, w, h)
    sd = helpers.scene_data(name)
    sob, sr = synth.blue_noise_tables()
    zbp = synth.z_buffer_params()
    op, rp = oracle.ShadowsPass(w, h), rh.RefShadowsPass(w, h)
    oa, ra = oracle.AOPass(w, h, zbp=zbp), rh.RefAOPass(w, h, zbp)
    lo, hi = sd.bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 3, 3), rays_per_probe=32, normal_bias=1.0 if name == "cornell" else 0.1)
    sky = synth_env.sky_cubemap(8)
    env = dict(sky=sky, prefiltered=synth_env.prefiltered_chain(sky, 4), pre_size=8, pre_levels=4, lut=synth_env.brdf_lut(8))
    dp, orp, rrp = od.DDGIPass(ddgi), orf.ReflectionsPass(w, h), rh.RefReflectionsPass(w, h, sd)
    rng = np.random.RandomState(7)
    gbr = [rc.reflections_variant(fr["gb"], checker=f in (rc.FRAME_H, rc.FRAME_C)) for f, fr in enumerate(frames)]
    for f, fr in enumerate(frames):
        cur, prev = fr["gb"], frames[f - 1 if f else 0]["gb"]
        for o, r in ((op, rp), (oa, ra)):
            o.render(osc, fr["ubo"], cur, prev, sob, sr, f)
            r.render(osc, fr["ubo"], cur, prev, sob, sr, f)
        a, b = op.stages, rp.stages
        for k in ("mask", "temporal", "moments", "tiles"):
            assert np.array_equal(a[k], b[k]), _where(info, a[k], b[k], f"shadows frame {f}: {k}")
        for i, (x, y) in enumerate(zip(a["atrous"], b["atrous"])):
            assert np.array_equal(x, y), f"shadows frame {f}: a-trous iteration {i}"
        c, d = oa.stages, ra.stages
        assert np.array_equal(c["mask"][0], d["mask"]), f"AO frame {f}: mask"
        for k in ("temporal", "length", "tiles", "blur0", "blur1"):
            assert np.array_equal(c[k], d[k]), _where(info, c[k], d[k], f"AO frame {f}: {k}")
        cur, prev = gbr[f], gbr[f - 1 if f else 0]
        dp.render(osc, fr["ubo"], cur, sky, synth_env.random_orientation(rng), f)
        irr, dep = dp.current_read()
        cd = (0.0, 0.0, 0.0) if f == 0 else (-1.0, 0.0, 0.0)
        orp.render(osc, fr["ubo"], ddgi, cur, prev, sob, sr, f, env, irr, dep, camera_delta=cd)
        rrp.render(osc, fr["ubo"], ddgi, cur, prev, sob, sr, f, env, irr, dep, camera_delta=cd)
        for k in ("trace", "temporal", "moments", "tiles", "output"):
            assert np.array_equal(orp.stages[k], rrp.stages[k]), _where(info, orp.stages[k], rrp.stages[k], f"reflections frame {f}: {k}")
        for i, (x, y) in enumerate(zip(orp.stages["atrous"], rrp.stages["atrous"])):
            assert np.array_equal(x, y), f"reflections frame {f}: a-trous iteration {i}"


def _where(info, a, b, what):
    if a.shape[:2] != info["family"].shape:
        return what
    bad = np.argwhere((a != b).reshape(a.shape[0], a.shape[1], -1).any(-1))
    return f"{what}: {len(bad)} pixels differ; first: " + "; ".join(rc.describe(info, int(y), int(x)) for y, x in bad[:4])
