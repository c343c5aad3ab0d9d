"""The crafted inputs of tests/closest_cases.py, checked without a GPU, so that tests/test_gpu_closest_edges.py and
tests/test_gpu_probe_update_edges.py cannot pass vacuously.  The REFERENCE is sound: the oracle's reflections and DDGI trace passes give the
same images and ray counts when every query walks its BVH and when every query tests every triangle (orc_scene_set_brute_force: primary
rays, the hit shader's light and sky rays) — tests/test_ref_shaders.py stays the arbiter of the shading itself.  And the cases are what they
say: every named family is there, every knife family takes both outcomes on at least a quarter of its rays under brute force, a different
winner among the triangles of a tie gives different stored bits, the listed tile and wave shapes exist, closed fans, shared edges and
doubled triangles are watertight."""
import functools

import numpy as np
import pytest

import closest_cases as cc
from hybrid_rendering_amd import synth


# ---------------------------------------------------------------------------------------------------------------- references (shared with the GPU files)
def _winner(osc, rays8):
    """brute-force closest hit of a ray batch [n][8] (origin, t_max, direction, t_min) -> (tuv, prim)"""
    return osc.closest_hit(np.ascontiguousarray(rays8, np.float32), brute_force=True)


def ddgi_reference(case, osc, brute=True):
    """(radiance, direction / distance, ray count) of the oracle's trace pass over the case's probes; untraced probes keep the sentinel"""
    from oracle import pyoracle_ddgi as od
    d = case["ddgi"]
    irr, dep = cc.coded_atlases(d)
    slab = int(d["probe_counts"][0]) * int(d["probe_counts"][1])
    probes = None if case["shard"] is None else (case["shard"][0] * slab, case["shard"][1] * slab)
    osc.set_brute_force(brute)
    try:
        return od.ray_trace(osc, cc.plain_ubo(case["light"]), d, case["orientation"], 0, bool(case["infinite_bounces"]) and not case["first"], 1.7, cc.coded_sky(),
                            irr, dep, probes=probes, fill=cc.SENTINEL)
    finally:
        osc.set_brute_force(False)


@functools.lru_cache(maxsize=1)
def ddgi_references():
    """[(case, oracle scene, dict(rad, dd, count, prim [probe][ray], won))]: computed once"""
    from oracle import pyoracle as po
    out, scenes = [], {}
    for c in cc.built_ddgi():
        osc = scenes.setdefault(id(c["sd"]), po.Scene(c["sd"]))
        rad, dd, count = ddgi_reference(c, osc)
        tuv, prim = _winner(osc, c["rays"].reshape(-1, 8))
        prim = prim.reshape(c["family"].shape)
        own = c["own"]
        won = (own[..., 0] >= 0) & (prim >= own[..., 0]) & (prim < own[..., 0] + own[..., 1])
        # closed: the construct won, or something nearer than it did (another ray's construct in the way)
        closed = won | ((prim >= 0) & (tuv[:, 0].reshape(prim.shape) < c["tdist"]))
        out.append((c, osc, dict(rad=rad, dd=dd, count=count, prim=prim, won=won, closed=closed)))
    return out


def refl_inputs(group):
    """the probe grid, its position-coded atlases and the environment every frame of a group is traced with"""
    ddgi = cc.refl_ddgi(group["sd"])
    irr, dep = cc.coded_atlases(ddgi)
    return ddgi, irr, dep, cc.coded_env()


def refl_reference(group, f, osc, brute=True):
    from oracle import pyoracle_reflections as orf
    ddgi, irr, dep, env = refl_inputs(group)
    sob, sr = synth.blue_noise_tables()
    osc.set_brute_force(brute)
    try:
        return orf.ray_trace(osc, f["ubo"], ddgi, dict(depth=f["depth"], gb2=f["gb2"], gb3=f["gb3"]), sob, sr, cc.trace_params(f["params"]), env, irr, dep)
    finally:
        osc.set_brute_force(False)


@functools.lru_cache(maxsize=1)
def refl_references():
    """[(group, oracle scene, [(frame, dict(trace, count, rays, prim, won))])]"""
    from oracle import pyoracle as po
    out = []
    for g in cc.built_reflections():
        osc = po.Scene(g["sd"])
        frames = []
        for f in g["frames"]:
            trace, count = refl_reference(g, f, osc)
            rays = cc.frame_rays(f)
            q = rays.reshape(-1, 8).copy()
            off = q[:, 7] == 0
            q[:, 3], q[:, 7] = 10000.0, 0.001
            q[off, 3] = 0.0
            q[off, 4:7] = (0.0, 0.0, 1.0)
            tuv, prim = _winner(osc, q)
            prim = prim.reshape(rays.shape[:2])
            prim[off.reshape(prim.shape)] = -1
            own = f["own"]
            won = (own[..., 0] >= 0) & (prim >= own[..., 0]) & (prim < own[..., 0] + own[..., 1])
            closed = won | ((prim >= 0) & (tuv[:, 0].reshape(prim.shape) < f["tdist"]))
            frames.append((f, dict(trace=trace, count=count, rays=rays, prim=prim, won=won, closed=closed)))
        out.append((g, osc, frames))
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference is sound
def test_ddgi_walk_equals_brute_force_on_every_case(oracle):
    total = 0
    for c, osc, r in ddgi_references():
        rad, dd, count = ddgi_reference(c, osc, brute=False)
        assert count == r["count"], (c["name"], count, r["count"])
        assert np.array_equal(rad, r["rad"]) and np.array_equal(dd, r["dd"]), f"{c['name']}: the oracle's BVH walk and its brute force differ in {int((rad != r['rad']).sum() + (dd != r['dd']).sum())} halfs"
        total += count
        print(f"{c['name']}: {c['rays'].shape[0]} x {c['rays'].shape[1]} probe rays, {count} rays with the hit shaders', {c['sd'].n_tris} triangles, hit fraction {float((r['prim'] >= 0).mean()):.3f}")
    assert total > 10000


def test_reflections_walk_equals_brute_force_on_every_frame(oracle):
    total = 0
    for g, osc, frames in refl_references():
        for f, r in frames:
            trace, count = refl_reference(g, f, osc, brute=False)
            assert count == r["count"], (f["name"], count, r["count"])
            assert np.array_equal(trace, r["trace"]), f"{f['name']}: the oracle's BVH walk and its brute force differ in {int((trace != r['trace']).sum())} halfs"
            traced = r["rays"][..., 7] != 0
            total += count
            assert count - int(traced.sum()) >= 0.5 * int((r["prim"][traced] >= 0).sum()), f"{f['name']}: few hits fire a light ray (the light must stand on the side the constructs face)"
            print(f"{g['name']}/{f['name']}: {int(traced.sum())} reflection rays, {count} with the light rays, {g['sd'].n_tris} triangles, hit fraction {float((r['prim'][traced] >= 0).mean()):.3f}")
            assert np.isfinite(cc.f16(r["trace"])).all()
    assert total > 8000


def test_gen_rays_are_the_rays_the_passes_trace(oracle):
    """the direction / distance image of the DDGI pass holds fp16(direction) of gen_rays; a reflections pixel has ray_length -1 exactly where
    gen_rays says sky / rough / a miss, and the ray counts are the traced flags plus the hit shaders' rays"""
    for c, osc, r in ddgi_references():
        if c["shard"] is None:
            assert np.array_equal(r["dd"][..., 0:3], cc.half(c["rays"][..., 4:7])), c["name"]
            assert r["count"] >= c["rays"].shape[0] * c["rays"].shape[1]
    for g, osc, frames in refl_references():
        for f, r in frames:
            h, w = f["h"], f["w"]
            traced = r["rays"][:h, :w, 7] != 0
            hit = traced & (r["prim"][:h, :w] >= 0)
            assert np.array_equal(cc.f16(r["trace"][..., 3]) != -1.0, hit), f["name"]
            assert r["count"] >= int(traced.sum()) and not (r["rays"][..., 7][r["rays"][..., 3] == cc.NO_THREAD]).any()


# ---------------------------------------------------------------------------------------------------------------- the cases are what they say
def _family_outcomes_ddgi(key="won"):
    fam = {}
    for c, osc, r in ddgi_references():
        if c["shard"] is not None or not c["first"] or c["infinite_bounces"]:
            continue        # the same rays again
        for i, n in enumerate(c["names"]):
            sel = c["family"] == i
            if sel.any():
                fam.setdefault(n, []).append(r[key][sel])
    return {k: np.concatenate(v) for k, v in fam.items()}


def test_ddgi_families(oracle):
    fam = _family_outcomes_ddgi()
    missing = [n for n in cc.DDGI_FAMILIES if n not in fam]
    assert not missing, missing
    for n, o in sorted(fam.items()):
        print(f"ddgi/{n}: {len(o)} rays, own construct wins {float(o.mean()):.3f}")
    for n in ("tmin", "tmax", "vertex", "edge", "backface", "rot_vertex"):
        assert len(fam[n]) >= 100 and 0.25 <= fam[n].mean() <= 0.75, (n, len(fam[n]), float(fam[n].mean()))
    closed = _family_outcomes_ddgi("closed")
    for n in ("shared_edge", "hub", "pair", "rot_shared_edge", "rot_hub", "rot_pair", "all_hit"):
        assert closed[n].all() and fam[n].mean() > 0.98, f"{n}: {int((~closed[n]).sum())} rays leak"
    assert not fam["zero_area"].any()
    for c, osc, r in ddgi_references():
        if "all_miss" in c["names"]:
            assert (r["prim"][c.of("all_miss")] == -1).all(), c["name"]
            assert (r["prim"][c.of("all_hit")] >= 0).all()
        if "coplanar_tri" in c:
            assert not (r["prim"] == c["coplanar_tri"]).any(), "a ray in a triangle's plane hits it"
        assert len(c["sd"].verts) <= 10000


def test_ddgi_wave_shapes_and_probe_positions(oracle):
    names = {c["name"]: (c, r) for c, _, r in ddgi_references()}
    for n, (c, r) in names.items():
        R, slab = c["rays"].shape[1], int(c["ddgi"]["probe_counts"][0]) * int(c["ddgi"]["probe_counts"][1])
        n_probes = c["rays"].shape[0] if c["shard"] is None else (c["shard"][1] - c["shard"][0]) * slab
        c["wave_facts"] = dict(straddles=R % 64 != 0 and n_probes * R > 64, partial=(n_probes * R) % 64 != 0)
    assert names["rot_r37"][0]["wave_facts"] == dict(straddles=True, partial=True) and names["rot_r100"][0]["wave_facts"] == dict(straddles=True, partial=True)
    assert names["scaled_r1"][0]["rays"].shape[1] == 1 and names["axis_3x2x2_r64"][0]["wave_facts"] == dict(straddles=False, partial=False)
    assert names["rot_r37_shard"][0]["shard"][0] > 0 and names["rot_r37_shard"][0]["wave_facts"]["partial"]
    sh, full = names["rot_r37_shard"][1], names["rot_r37"][1]
    assert (sh["rad"][:6] == cc.SENTINEL).all() and np.array_equal(sh["rad"][6:], full["rad"][6:]) and 0 < sh["count"] < full["count"]
    later = names["rot_r37_later"][1]
    assert not np.array_equal(later["rad"], full["rad"]) and np.array_equal(later["dd"], full["dd"]), "infinite bounces change the radiance only"
    fi = names["rot_r100_first_inf"][1]
    assert np.array_equal(fi["rad"], names["rot_r100"][1]["rad"]), "the first frame ignores infinite_bounces"
    # the scaled rotation is no rotation, and its directions still come out unit; the box-plane grid starts on three planes of one child box
    s = names["scaled_r1"][0]
    assert abs(np.linalg.norm(s["orientation"].reshape(3, 3)[0]) - 2.5) < 1e-3 and np.abs(np.linalg.norm(s["rays"][..., 4:7], axis=-1) - 1).max() < 1e-6
    b = names["box_planes"][0]
    assert np.array_equal(b["rays"][0, 0, 0:3], b["box"]["lo"]) and 0.2 < (names["box_planes"][1]["prim"] >= 0).mean() < 0.95
    # a probe in the plane of a triangle around it
    c, r = names["rot_r37"]
    assert (c["sd"].verts[:, :, 2] == c["rays"][7, 0, 2]).all(1).any(), "no triangle in the plane of probe 7"


def test_ddgi_stored_distances_land_on_fp16_rounding_ties(oracle):
    """behind the t_min covers of the axis cases: hits whose 0.001f + t is EXACTLY halfway between two fp16 values (the stored distance must be
    the even neighbour), and one fp32 ulp to either side of such a midpoint (it must be the nearer one)"""
    ties = below = above = down = up = 0
    for c, osc, r in ddgi_references():
        if not c.get("tie_tris") or c["shard"] is not None or not c["first"]:
            continue
        hit = np.isin(r["prim"], c["tie_tris"]) & (c["rays"][..., 6] == 1) & (c["rays"][..., 2] == 0)      # the bottom slab's own rays (a top probe's down ray may land there too)
        z = c["sd"].verts[r["prim"][hit], 0, 2]                       # the cover's height is t itself: origin z == 0, d.z == 1
        total = (np.float32(0.001) + z).astype(np.float32)
        stored = r["dd"][..., 3][hit].view(np.float16)
        assert np.array_equal(stored, total.astype(np.float16)), c["name"]
        lo = np.floor((total.astype(np.float64) - 1.0) * 1024.0) / 1024.0 + 1.0
        mid = lo + 2.0 ** -11
        ties += int((total == mid).sum()); below += int((total < mid).sum()); above += int((total > mid).sum())
        on = total == mid
        down += int((on & (stored.astype(np.float64) == lo)).sum()); up += int((on & (stored.astype(np.float64) > lo)).sum())
    print(f"stored distances on an fp16 tie: {ties} ({down} round down to the even neighbour, {up} up), an fp32 ulp below: {below}, above: {above}")
    assert ties >= 100 and down >= 20 and up >= 20 and below >= 50 and above >= 50


def test_ddgi_tie_winners_are_told_apart_by_the_stored_bits(oracle):
    """within a tie family (doubled triangles, fans, shared edges: several triangles at the same t) the map winning primitive -> stored radiance
    is injective over the family's rays of one probe-and-direction group, so a walk that returns another winner changes stored bits"""
    checked = 0
    for c, osc, r in ddgi_references():
        if c["shard"] is not None or not c["first"]:
            continue
        for n in ("pair", "hub", "shared_edge", "rot_pair", "rot_hub", "rot_shared_edge"):
            if n not in c["names"]:
                continue
            sel = c.of(n)
            own, prim, rad = c["own"][sel], r["prim"][sel], r["rad"][sel]
            # every triangle of the winner's construct, shaded at the same point, must give other bits than the winner: compare the materials'
            # albedo (the only thing that differs between the triangles of a pair; fans and shared edges also differ in the normal)
            m = c["sd"].materials
            for (first, cnt), p in zip(own[:: max(1, len(own) // 50)], prim[:: max(1, len(own) // 50)]):
                others = [q for q in range(first, first + cnt) if q != p]
                assert all(np.abs(cc.half(m[q, 0:3]).astype(np.int32) - cc.half(m[p, 0:3]).astype(np.int32)).max() >= 8 for q in others), (c["name"], n, p)
                checked += 1
        # and directly: over the tie families' hit rays of a case, stored radiance bits -> winning primitive is a function (no two primitives
        # share a stored colour), for the rays whose radiance is not all zero (an unlit metallic hit stores 0 whatever its albedo)
        ties = np.zeros(c["family"].shape, bool)
        for n in ("pair", "hub", "shared_edge", "rot_pair", "rot_hub", "rot_shared_edge"):
            if n in c["names"]:
                ties |= c.of(n)
        ties &= r["prim"] >= 0
        lit = ties & (r["rad"][..., 0:3] != 0).any(-1)
        assert lit.sum() >= 0.9 * ties.sum(), (c["name"], int(lit.sum()), int(ties.sum()))
        by_colour = {}
        for p, bits in zip(r["prim"][lit], r["rad"][lit][:, 0:3]):
            by_colour.setdefault(bits.tobytes(), set()).add(int(p))
        assert all(len(v) == 1 for v in by_colour.values()), (c["name"], [v for v in by_colour.values() if len(v) > 1][:4])
    assert checked > 100


def _refl_family_outcomes(key="won"):
    fam, regime = {}, {}
    for g, osc, frames in refl_references():
        for f, r in frames:
            if not f.get("aimed"):
                continue
            traced = r["rays"][..., 7] != 0
            for i, n in enumerate(f["names"]):
                sel = f["family"] == i
                if sel.any():
                    fam.setdefault(n, []).append(r[key][sel & traced])
                    regime.setdefault(n, []).append(r["rays"][..., 3][sel])
    return {k: np.concatenate(v) for k, v in fam.items()}, {k: np.concatenate(v) for k, v in regime.items()}


def test_reflection_families(oracle):
    fam, regime = _refl_family_outcomes()
    missing = [n for n in cc.REFL_FAMILIES if n not in fam]
    assert not missing, missing
    for n, o in sorted(fam.items()):
        print(f"reflections/{n}: {len(regime[n])} threads, {len(o)} rays, own construct wins {float(o.mean()) if len(o) else float('nan'):.3f}")
    for n in ("rot_vertex", "rot_vertex_ragged", "tmin", "tmax"):
        assert len(fam[n]) >= 100 and 0.25 <= fam[n].mean() <= 0.75, (n, len(fam[n]), float(fam[n].mean()))
    closed, _ = _refl_family_outcomes("closed")
    for n in ("rot_shared_edge", "rot_hub", "rot_pair", "rot_pair_ragged", "rot_hub_ragged", "rot_shared_edge_ragged"):
        assert len(fam[n]) and closed[n].all() and fam[n].mean() > 0.98, f"{n}: {int((~closed[n]).sum())} rays leak"
    for n in cc.ODDITIES:        # every ray set-up oddity also through a HIT (the same triangle twice across its ray)
        assert len(fam[n + "_hit"]) >= 12 and fam[n + "_hit"].all(), n
    assert not fam["sky_seam"].any() and not fam["sky_seam_beside"].any() and len(fam["length_tie"]) >= 200 and fam["length_tie"].all()


def test_reflection_sky_seams_and_ray_length_ties(oracle):
    """sky_seams: misses whose direction has |x| == z or |y| == z EXACTLY (the larger of the two; the seam between a side face and +Z of the sky
    cube), where the pinned rule takes the side face (x over y over z, `>=`), and, a depth ulp beside, directions on either side of the seam;
    the stored colour of the position-coded sky names the face.  length_ties: hits whose 0.001f + t is EXACTLY halfway between two fp16 values
    (the stored ray_length is the even neighbour) and one fp32 ulp to either side (the nearer one)."""
    refs = {f["name"]: (f, r) for g, _, frames in refl_references() for f, r in frames}
    f, r = refs["sky_seams"]
    h, w = f["h"], f["w"]
    d = r["rays"][:h, :w, 4:7]
    on = f.of("sky_seam")[:h, :w]
    side = np.maximum(np.abs(d[..., 0]), np.abs(d[..., 1]))
    assert on.sum() >= 300 and (side[on] == d[..., 2][on]).all() and (r["prim"][:h, :w][on] == -1).all(), "a seam ray is not exactly on the seam, or hits"
    assert (np.abs(d[..., 0])[on] == d[..., 2][on]).sum() >= 100 and (np.abs(d[..., 1])[on] == d[..., 2][on]).sum() >= 20
    face = np.round((cc.f16(r["trace"][..., 0]) - 0.05) / 0.1).astype(int)          # coded_sky: red = 0.05 + 0.1 * face
    want = np.where(np.abs(d[..., 0]) >= np.abs(d[..., 1]), np.where(d[..., 0] >= 0, 0, 1), np.where(d[..., 1] >= 0, 2, 3))
    assert np.array_equal(face[on], want[on]), "on the seam the side face wins"
    near = f.of("sky_seam_beside")[:h, :w]
    above, below = near & (d[..., 2] > side), near & (d[..., 2] < side)
    assert above.sum() >= 100 and below.sum() >= 100 and (face[above] == 4).all() and np.array_equal(face[below], want[below])
    print(f"sky seams: {int(on.sum())} rays exactly on a seam, {int(above.sum())} just on the +Z side, {int(below.sum())} just on the side face's")
    # the seam between two side faces: |d.x| == |d.y| > |d.z| exactly; x wins the tie; a depth ulp beside, the larger of the two does
    f, r = refs["sky_seams_xy"]
    d = r["rays"][:h, :w, 4:7]
    ax, ay, az = np.abs(d[..., 0]), np.abs(d[..., 1]), np.abs(d[..., 2])
    on, near = f.of("sky_seam_xy")[:h, :w], f.of("sky_seam_xy_beside")[:h, :w]
    assert on.sum() >= 200 and (ax[on] == ay[on]).all() and (ax[on] > az[on]).all() and (r["prim"][:h, :w][on | near] == -1).all()
    face = np.round((cc.f16(r["trace"][..., 0]) - 0.05) / 0.1).astype(int)
    fx, fy = np.where(d[..., 0] >= 0, 0, 1), np.where(d[..., 1] >= 0, 2, 3)
    assert np.array_equal(face[on], fx[on]), "on the x / y seam the X face wins"
    more_y, more_x = near & (ay > ax), near & (ay < ax)
    assert more_y.sum() >= 50 and more_x.sum() >= 50 and np.array_equal(face[more_y], fy[more_y]) and np.array_equal(face[more_x], fx[more_x])
    print(f"sky seams between side faces: {int(on.sum())} rays exactly on |x| == |y|, {int(more_y.sum())} just on the Y face's side, {int(more_x.sum())} just on the X face's")
    f, r = refs["length_ties"]
    stored = r["trace"][..., 3].view(np.float16)
    total = f["want"][:h, :w]
    tie, beside = f.of("length_tie")[:h, :w], f.of("length_tie_beside")[:h, :w]
    assert (total[tie | beside] != 0).all() and np.array_equal(stored[tie | beside], total[tie | beside].astype(np.float16))
    lo = np.floor((total.astype(np.float64) - 1.0) * 1024.0) / 1024.0 + 1.0
    mid = lo + 2.0 ** -11
    assert (total[tie] == mid[tie]).all() and (total[beside] != mid[beside]).all()
    down, up = int((stored[tie].astype(np.float64) == lo[tie]).sum()), int((stored[tie].astype(np.float64) > lo[tie]).sum())
    print(f"ray_length on an fp16 tie: {int(tie.sum())} ({down} round down to the even neighbour, {up} up), an fp32 ulp beside: {int(beside.sum())}")
    assert tie.sum() >= 200 and down >= 50 and up >= 50 and (total[beside] < mid[beside]).sum() >= 100 and (total[beside] > mid[beside]).sum() >= 100
    # GGX at roughness 0.05-and-a-code and 1.0 crossed with trim 0 / 0.8 / 1: the rays of those pixels differ between the three frames
    ggx = f.of("ggx_rough_min_hit") | f.of("ggx_rough_one_hit")
    assert ggx.sum() >= 30 and (r["rays"][..., 3][ggx] == cc.GGX).all()
    d08, d0, d1 = (refs[n][1]["rays"][..., 4:7][ggx] for n in ("length_ties", "oddities_trim0", "oddities_trim1"))
    assert (d0 != d08).any(1).mean() > 0.9 and (d1 != d08).any(1).mean() > 0.9 and (d1 != d0).any(1).mean() > 0.9


def test_reflection_regimes_and_tile_shapes(oracle):
    refs = {f["name"]: (f, r) for g, _, frames in refl_references() for f, r in frames}
    f, r = refs["tiles"]
    reg, traced = r["rays"][..., 3], r["rays"][..., 7] != 0
    t = lambda tx, ty: cc._tile(tx, ty)
    assert (reg[t(0, 0)] == cc.SKY).all() and (reg[t(1, 0)] == cc.DDGI_ROUGH).all() and not traced[t(1, 0)].any()
    assert traced[t(2, 0)].sum() == 1 and traced[t(3, 0)].sum() == 64
    assert traced[t(4, 0)].sum() == 63 and (reg[t(4, 0)] == cc.DDGI_ROUGH).sum() == 1
    assert traced[t(5, 0)].sum() == 1 and (reg[t(5, 0)] == cc.DDGI_ROUGH).sum() == 63
    # ragged tiles: off-image lanes are no threads, the in-image lanes all trace
    assert (reg[:, 61:] == cc.NO_THREAD).all() and (reg[45:, :] == cc.NO_THREAD).all() and (reg[:45, :61] != cc.NO_THREAD).all()
    assert traced[24:45, 56:61].mean() > 0.9 and traced[40:45, 24:56].mean() > 0.9 and not traced[24:45, 56:61].all()      # a rough lane among them
    # two ragged tiles in which only the image's last column / last row has geometry: 8 tracing lanes among sky lanes and no-thread lanes
    for tile, edge in ((t(7, 2), np.s_[16:24, 60]), (t(2, 5), np.s_[44, 16:24])):
        assert traced[tile].sum() == 8 and traced[edge].all() and (reg[tile] == cc.SKY).sum() > 0 and (reg[tile] == cc.NO_THREAD).sum() >= 24
        assert (f["family"][tile] == f["names"].index("tile_ragged_edge_only")).all()
    # the regime ties: with approximate_with_ddgi the codes split three ways, without it two ways; each regime holds >= 25 % of the family
    ties = reg[t(6, 0)]
    lo, hi = cc.roughness_codes()
    rough = cc.f16(f["gb3"][0:8, 48:56, 0])
    want = np.where(rough < np.float32(0.05), cc.MIRROR, np.where(rough > np.float32(0.75), cc.DDGI_ROUGH, cc.GGX))
    assert np.array_equal(ties, want) and all((ties == k).mean() >= 0.25 for k in (cc.MIRROR, cc.GGX, cc.DDGI_ROUGH)), [float((ties == k).mean()) for k in (1, 2, 3)]
    assert lo[1] < np.float32(0.05) < lo[2] and hi[1] == 0.75
    f0, r0 = refs["tiles_approx0_gi0"]
    ties0 = r0["rays"][..., 3][t(6, 0)]
    assert np.array_equal(ties0, np.where(rough < np.float32(0.05), cc.MIRROR, cc.GGX)) and (ties0 == cc.MIRROR).mean() >= 0.25 and (ties0 == cc.GGX).mean() >= 0.25
    # trim moves the GGX rays and no other
    ggx = reg == cc.GGX
    for n in ("tiles_trim0", "tiles_trim1"):
        d1 = refs[n][1]["rays"][..., 4:7]
        assert (d1[ggx] != r["rays"][..., 4:7][ggx]).any(1).mean() > 0.9 and np.array_equal(d1[reg == cc.MIRROR], r["rays"][..., 4:7][reg == cc.MIRROR])
    # the interval frame: origins in the plane z == 0, one pixel looks straight down its normal, the oddities are where they say
    f, r = refs["interval"]
    assert (r["rays"][2:f["h"], :f["w"], 2] == 0).all() and np.array_equal(r["rays"][18, 26, 4:7], np.float32([0, 0, 1]))
    assert (r["rays"][..., 3][f.of("depth_below_one")] != cc.SKY).all() and (r["rays"][..., 3][f.of("depth_above_one")] != cc.SKY).all()
    away = r["rays"][f.of("normal_away")]
    assert (away[:, 6] > 0.99).all(), "N = (0,0,-1) under a camera above (N.Wo ~ -1): the mirror direction is -Wo + 2 (N.Wo) N, upwards again"
    across = r["rays"][f.of("normal_across")]
    assert (np.abs(across[:, 4]) < 0.1).all() and (across[:, 6] < -0.99).all(), "N = (1,0,0) (N.Wo ~ 0): the mirror ray runs down, away from every cover"
    assert (r["rays"][..., 3][f.of("ggx_rough_min")] == cc.GGX).all() and (r["rays"][..., 3][f.of("ggx_rough_one")] == cc.GGX).all()
    assert np.signbit(f["depth"]).any() and (f["depth"] > 1).any()


def test_reflection_colours_stay_under_the_clamp_and_name_the_winner(oracle):
    """hit pixels keep every channel under 0.7 (the clamp would hide the winner), and in the tie families (the same triangle twice, fans, shared
    edges) the winner's material differs from its construct's other materials by far more than an fp16 ulp of the colour"""
    checked = 0
    for g, osc, frames in refl_references():
        m = g["sd"].materials
        for f, r in frames:
            h, w = f["h"], f["w"]
            hit = (r["prim"][:h, :w] >= 0) & (r["rays"][:h, :w, 7] != 0)
            rgb = cc.f16(r["trace"][..., 0:3])
            assert not hit.any() or rgb[hit].max() < 0.7, (f["name"], float(rgb[hit].max()))
            # directly: over the tie families' hits (ragged and row-0 constructs included: every construct of more than one triangle), stored colour
            # bits -> winning primitive is a function, and every such hit is lit (not all zero)
            ties = hit & (f["own"][:h, :w, 1] > 1)
            if ties.any():
                lit = ties & (r["trace"][..., 0:3] != 0).any(-1)      # a hit in another construct's shadow stores 0 where sample_gi is off
                print(f"{f['name']}: {int(ties.sum())} tie hits, {int(lit.sum())} lit")
                assert lit.sum() >= 0.9 * ties.sum(), (f["name"], int(lit.sum()), int(ties.sum()))
                if f["params"]["sample_gi"]:
                    assert lit.sum() == ties.sum(), (f["name"], "with sample_gi every hit stores a colour")
                bits = r["trace"][..., 0:3][lit]
                by_colour = {}
                for p, b in zip(r["prim"][:h, :w][lit], bits):
                    by_colour.setdefault(b.tobytes(), set()).add(int(p))
                assert all(len(v) == 1 for v in by_colour.values()), (f["name"], [v for v in by_colour.values() if len(v) > 1][:4])
            if not f.get("aimed"):
                continue
            for n in ("rot_pair", "rot_hub", "rot_shared_edge"):
                if n not in f["names"]:
                    continue
                sel = f.of(n)[:h, :w] & hit
                for (first, cnt), p in zip(f["own"][:h, :w][sel][::7], r["prim"][:h, :w][sel][::7]):
                    others = [q for q in range(first, first + cnt) if q != p]
                    assert all(np.abs(cc.half(m[q, 0:3]).astype(np.int32) - cc.half(m[p, 0:3]).astype(np.int32)).max() >= 8 for q in others)
                    checked += 1
    assert checked > 50


# ---------------------------------------------------------------------------------------------------------------- probe update
def test_update_cases_cover_the_listed_sizes(oracle):
    ties = [c for c in cc.update_cases() if c["name"].startswith("tie")]
    assert len(ties) == 2 and all({cc.UPDATE_FAMILIES[i] for i in c["family"]} == {"exact_tie"} for c in ties)
    cases = [c for c in cc.update_cases() if not c["name"].startswith("tie")]
    d = [c["ddgi"] for c in cases]
    assert sorted(c["R"] for c in cases) == [1, 3, 255, 256, 257, 513]
    assert sorted(int(u["depth_probe_side_length"]) for u in d) == [2, 8, 9, 11, 12, 16] and sorted(set(int(u["irradiance_probe_side_length"]) for u in d)) == [2, 7, 8, 16]
    assert sorted(set(((int(u["depth_probe_side_length"]) ** 2 + 63) // 64) * 64 for u in d)) == [64, 128, 192, 256]
    assert {float(u["hysteresis"]) for u in d} == {0.0, 1.0, np.float32(0.98)} and {float(u["depth_sharpness"]) for u in d} == {50.0, 37.0}
    assert any(c["first"] for c in cases) and any(not c["first"] for c in cases) and any(c["shard"] and c["shard"][0] > 0 for c in cases)
    for c in cases:
        assert all(np.isfinite(cc.f16(c[k])).all() for k in ("rad", "dd", "prev_irr", "prev_dep"))
        assert set(cc.UPDATE_FAMILIES) - {"exact_tie"} == {cc.UPDATE_FAMILIES[i] for i in c["family"]}
    dist = np.concatenate([cc.f16(c["dd"][..., 3]).reshape(-1) for c in cases])
    for v in (0.0, -1.0, 10000.0):
        assert (dist == v).any(), v
    assert (np.signbit(dist) & (dist == 0)).any()
    m = cases[2]["ddgi"]["max_distance"]
    around = cc.f16(cases[2]["dd"][..., 3])[cases[2]["family"] == cc.UPDATE_FAMILIES.index("distances")]
    assert ((around - np.float32(0.01)) > m).any() and ((around - np.float32(0.01)) < m).any()


def test_update_knives_take_both_outcomes(oracle):
    """the aimed (texel, ray) pairs: the restated weight is >= 1e-8 on the `taken` side and below on the other, within 5 % of the threshold for the
    depth atlas (sharpness 50 and 37) and within a factor of 8 for the irradiance atlas, whose fp16 SUBNORMAL directions offer no finer step;
    half of each family on either side"""
    for c in cc.update_cases():
        if c["name"].startswith("tie"):
            continue        # exactly ON the threshold: test_weights_exactly_on_the_threshold
        d = c["ddgi"]
        for atlas, side, sharp in ((0, int(d["irradiance_probe_side_length"]), None), (1, int(d["depth_probe_side_length"]), float(d["depth_sharpness"]))):
            a = c["aimed"]
            sel = a[..., 0] == atlas
            if not sel.any():
                continue
            t = cc.texel_dirs(side).reshape(-1, 3)[a[..., 1][sel]]
            w = cc.weight32(t, c["dirs"][sel], sharp)
            taken = w >= cc.EPS
            assert np.array_equal(taken, a[..., 2][sel] == 0), c["name"]
            print(f"{c['name']} atlas {atlas}: {int(sel.sum())} aimed pairs, taken {float(taken.mean()):.3f}, weight / 1e-8 in [{float(w[taken].min() / cc.EPS):.4f}, {float(w[taken].max() / cc.EPS):.4f}] taken, "
                  f"[{float(w[~taken].min() / cc.EPS):.4f}, {float(w[~taken].max() / cc.EPS):.4f}] skipped")
            if sel.sum() >= 8:
                assert 0.25 <= taken.mean() <= 0.75
            if atlas == 1:
                assert (w[taken] / cc.EPS).max() < 1.05 and (w[~taken] / cc.EPS).min() > 0.95      # half an fp16 ulp of the direction moves dp^50 by 1.2 %
            else:
                assert (w[taken] / cc.EPS).max() < 8.0


def test_weights_exactly_on_the_threshold(oracle):
    """`>=` against `>` at the 1e-8 thresholds needs a weight of EXACTLY 1e-8f.
    The exact_tie family has them: its directions give dot == 1e-8f bit for bit on their texel of side 12 — the irradiance weight, and with
    depth_sharpness 1 the depth weight.  Alone in its probe such a ray is TAKEN (w >= 1e-8) and the total weight, 1e-8, is NOT normalised
    (total_w > 1e-8 is false): the oracle's texel is fp16(0.95 * radiance * 1e-8), neither 0 (skipped) nor 0.95 * radiance (normalised).
    What stays out of reach, provably: with depth_sharpness 50 or 37 no fp32 x has det_powi(x, n) == 1e-8f (the power is monotone; a scan of
    4000 ulps to either side of the root crosses the threshold without landing on it), and `roughness < 0.05f` against `<=` (the G-buffer's
    roughness is fp16 and 0.05f is no fp16 value)."""
    T = cc.EPS
    td = cc.texel_dirs(cc.TIE_SIDE).reshape(-1, 3)
    for k, bits in cc.TIES:
        assert cc.weight32(td[k][None], cc.f16(np.array(bits, np.uint16))[None])[0] == T, (k, bits)
    assert len({k for k, _ in cc.TIES}) == 4
    for n in (50, 37):
        root = np.float32(1e-8 ** (1.0 / n))
        x = (root.view(np.uint32) + np.arange(-4000, 4001)).astype(np.uint32).view(np.float32)
        w = cc.powi32(x, n)
        assert (np.diff(w) >= 0).all() and w[0] < T < w[-1] and not (w == T).any(), n
    assert np.float32(np.float16(0.05)) != np.float32(0.05) and np.float32(np.float16(0.75)) == np.float32(0.75)
    c = [c for c in cc.update_cases() if c["name"] == "tie_r1"][0]
    irr, dep = cc.update_reference(c)
    counts = tuple(int(v) for v in c["ddgi"]["probe_counts"])
    for p in range(12):
        k = int(c["aimed"][p, 0, 1])
        rad = cc.f16(c["rad"][p, 0, 0:3])
        want = ((rad * np.float32(0.95)).astype(np.float32) * T).astype(np.float32).astype(np.float16)
        got = cc.interior(irr, cc.TIE_SIDE, counts, p).reshape(-1, 4)[k, 0:3].view(np.float16)
        assert np.array_equal(got, want) and (want[0:2] != 0).all(), (p, got, want)
        dgot = cc.interior(dep, cc.TIE_SIDE, counts, p).reshape(-1, 2)[k].view(np.float16)
        assert (dgot != 0).any(), "the depth texel of an exact tie with sharpness 1 is taken too"


def test_the_exact_ties_are_reproducible():
    """closest_cases.search_exact_ties finds the committed TIES on side 12 (all of them, on the same four texels) and nothing on the irradiance
    sides the listed cases use"""
    found = cc.search_exact_ties(cc.TIE_SIDE)
    assert set(cc.TIES) <= set(found) and {k for k, _ in found} == {k for k, _ in cc.TIES}, (found, cc.TIES)
    for side in (2, 7, 8, 16):
        assert cc.search_exact_ties(side) == [], side


def test_update_restatement_agrees_with_the_oracle_on_single_rays(oracle):
    """R == 1: a texel of the oracle's irradiance atlas is 0.95 * radiance exactly where the restated weight takes the probe's one ray, and 0 where it
    skips it (first frame: no history) — the restatement that aims the rays is the oracle's arithmetic"""
    c = cc.update_cases()[0]
    assert c["R"] == 1 and c["first"]
    irr, dep = cc.update_reference(c)
    d = c["ddgi"]
    counts = tuple(int(v) for v in d["probe_counts"])
    side = int(d["irradiance_probe_side_length"])
    seen = set()
    for p in range(int(np.prod(counts))):
        w = cc.weight32(cc.texel_dirs(side), c["dirs"][p, 0][None, None])
        got = cc.f16(cc.interior(irr, side, counts, p)[..., 0])
        want = np.where(w >= cc.EPS, (cc.f16(c["rad"][p, 0, 0]) * np.float32(0.95)).astype(np.float16).astype(np.float32), 0.0)
        assert np.array_equal(got, want), (p, got, want)
        seen |= set((w >= cc.EPS).reshape(-1).tolist())
    assert seen == {True, False}


def test_update_reference_keeps_the_sentinel_and_obeys_the_copy_rule(oracle):
    for c in cc.update_cases():
        irr, dep = cc.update_reference(c)
        d = c["ddgi"]
        counts = tuple(int(v) for v in d["probe_counts"])
        z0, z1 = c["shard"] if c["shard"] is not None else (0, counts[2])
        for atlas, side in ((irr, int(d["irradiance_probe_side_length"])), (dep, int(d["depth_probe_side_length"]))):
            rows = cc.cell_rows(side, z0, z1)
            assert (atlas[0] == cc.SENTINEL).all() and (atlas[-1] == cc.SENTINEL).all() and (atlas[:, 0] == cc.SENTINEL).all() and (atlas[:, -1] == cc.SENTINEL).all()
            inside = atlas[rows, 1:-1]
            assert not (inside == cc.SENTINEL).all(-1).any(), "a texel of a traced slab was not written"
            assert np.array_equal(cc.expect_borders(atlas, side, counts)[rows], atlas[rows]), (c["name"], "the oracle's borders differ from the copy rule")
            if c["shard"] is not None:
                outside = np.ones(atlas.shape[0], bool); outside[rows] = False
                assert (atlas[outside] == cc.SENTINEL).all()
    # all-skipped probes: nothing taken, nothing normalised; hysteresis 1 keeps the history bit for bit
    c = cc.update_cases()[0]
    irr, _ = cc.update_reference(c)
    p = int(np.flatnonzero(c["family"] == cc.UPDATE_FAMILIES.index("all_skipped"))[0])
    assert (cc.interior(irr, 2, (3, 2, 2), p)[..., 0:3] == 0).all()
    c = cc.update_cases()[2]
    irr, dep = cc.update_reference(c)
    for p in range(12):
        assert np.array_equal(cc.interior(irr, 8, (3, 2, 2), p)[..., 0:3], cc.interior(c["prev_irr"], 8, (3, 2, 2), p)[..., 0:3])
        assert np.array_equal(cc.interior(dep, 9, (3, 2, 2), p), cc.interior(c["prev_dep"], 9, (3, 2, 2), p))
