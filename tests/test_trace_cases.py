"""The adversarial G-buffers of tests/trace_cases.py, checked without a GPU, so that tests/test_gpu_trace_gbuffer_edges.py cannot pass
vacuously: every family is there, every knife family takes both outcomes under BRUTE FORCE on at least a quarter of its rays (the bar of
test_interval_knife_edges_match_brute_force), closed fans and shared edges are watertight, every tile shape exists, edge threads are both lit
and occluded — and the REFERENCE is sound: the oracle's BVH walk equals its brute force on every ray, and the oracle's own shadow and AO
trace passes produce exactly the packed brute-force bits and ray counts."""
import functools

import numpy as np
import pytest

import trace_cases as tc
from hybrid_rendering_amd import synth

SHADOW_FAMILIES = ("tile_all_sky", "tile_all_att0", "tile_one_lane", "tile_full", "tile_edge_only", "edge_thread", "fire_normals", "sky_ties",
                   "vertex", "edge", "backface", "shared_edge", "hub", "zero_area", "tmin", "tmax_dir", "coplanar", "tmax_point", "light_at_P",
                   "light_in_plane", "light_at_origin", "cone_outer", "cone_inner", "graze_plane", "graze_ulps", "graze_step", "graze_edge", "graze_edge_step")
AO_FAMILIES = ("interval_7", "interval_0.1", "interval_0.5", "cell_face", "below_lo", "above_hi", "at_hi", "at_hi_corner", "planar", "planar_in_plane",
               "far_interval_0.1", "far_interval_0.5", "aimed_0.1", "aimed_0.5")


def reference(osc, f, check_walk=False):
    """brute force over the exact rays of every thread of frame f: dict(rays, fired, occ (both [(spp)][ph][pw]), mask, count, tiles)"""
    rays = tc.frame_rays(f)
    q = tc.query_rays(rays)
    occ = osc.any_hit(q, brute_force=True)
    if check_walk:
        walk = osc.any_hit(q)
        assert np.array_equal(occ != 0, walk != 0), f"{f['name']}: the oracle's BVH walk and its brute force differ on {int(((occ != 0) != (walk != 0)).sum())} rays"
    fired = rays[..., 7] != 0
    occ = (occ.reshape(fired.shape) != 0) & fired
    mask, count, tiles = tc.expected(rays, occ)
    return dict(rays=rays, fired=fired, occ=occ, mask=mask, count=count, tiles=tiles)


@functools.lru_cache(maxsize=None)
def references(which):
    """[(group, oracle scene, [(frame, reference)])], computed once and shared (the GPU file imports it)"""
    from oracle import pyoracle as po
    out = []
    for g in tc.built(which):
        osc = po.Scene(tc.scene_data(g["tris"], g["name"]))
        out.append((g, osc, [(f, reference(osc, f, check_walk=True)) for f in g["frames"]]))
    return out


def all_frames(which):
    return [(g, f, r) for g, _, fr in references(which) for f, r in fr]


def outcome(f, r, name, kind):
    """the 0/1 outcomes of a family's rays: fired flags ("fire") or brute-force occlusion of the fired rays ("hit"; AO: the targeted sample)"""
    sel = f.of(name)
    if kind == "fire":
        return r["fired"][sel]
    if r["occ"].ndim == 3:
        if f.get("sample") is None or f["spp"] == 1:
            return r["occ"][:, sel][r["fired"][:, sel]]
        yy, xx = np.nonzero(sel)
        s = f["sample"][yy, xx]
        return r["occ"][s, yy, xx][r["fired"][s, yy, xx]]
    return r["occ"][sel & r["fired"]]


@pytest.mark.parametrize("which,want", (("shadows", SHADOW_FAMILIES), ("ao", AO_FAMILIES)))
def test_every_family_is_present_and_sizes_are_small(oracle, which, want):
    seen = {}
    for g, f, r in all_frames(which):
        assert (f["w"], f["h"]) in tc.SIZES and len(g["tris"]) <= 16000, (g["name"], len(g["tris"]))
        assert np.isfinite(f["depth"]).all() and f["depth"].max() <= 3.0 and f["depth"].min() >= 0.0
        for i, n in enumerate(f["names"]):
            seen[n] = seen.get(n, 0) + int((f["family"] == i).sum())
    missing = [n for n in want if seen.get(n, 0) == 0]
    assert not missing, missing
    if which == "shadows":
        d = np.concatenate([f["depth"].reshape(-1) for _, f, _ in all_frames(which)])
        for v in (np.float32(1.0), np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), np.float32(1.5)):
            assert (d == v).any(), v
        assert (np.signbit(d) & (d == 0)).any(), "-0"


@pytest.mark.parametrize("which", ("shadows", "ao"))
def test_knife_families_take_both_outcomes(oracle, which):
    fam = {}
    for g, f, r in all_frames(which):
        for name, kind in f["knife"].items():
            o = outcome(f, r, name, kind)
            print(f"{f['name']}/{name} ({kind}): {len(o)} rays, {float(o.mean()):.3f}")
            fam.setdefault((g["name"], name, kind), []).append(o)
    for key, o in fam.items():      # a family is its rays over every frame of its group (the light stepped by ulps: one frame per step)
        o = np.concatenate(o)
        assert len(o) >= 40 and 0.25 <= o.mean() <= 0.75, (key, len(o), float(o.mean()))
    assert len(fam) >= 8


def test_closed_fans_and_shared_edges_are_watertight(oracle):
    """every ray through the hub of a closed fan or a point of an edge two triangles share (exactly, and 1 .. 8 ulps beside it) is occluded;
    zero-area triangles on a ray never are"""
    g, f, r = all_frames("shadows")[0]
    assert f["name"] == "axis"
    for name in f["must_hit"]:
        sel = f.of(name)
        assert sel.sum() > 200 and (f["ulps"][sel] == 0).sum() > 20
        assert r["fired"][sel].all() and r["occ"][sel].all(), f"{name}: {int((~r['occ'][sel]).sum())} rays leak"
    assert not r["occ"][f.of("zero_area")].any()
    # the single triangles: a feature exactly on the ray decides one way for all of them, and both sides of it are populated
    for name in ("vertex", "edge", "backface"):
        sel = f.of(name)
        for k in tc.ULPS:
            assert (sel & (f["ulps"] == k)).sum() >= 20, (name, k)


def test_tile_shapes_exist(oracle):
    g, f, r = all_frames("shadows")[0]
    kind = tc.thread_kind(f["w"], f["h"])
    ph, pw = kind.shape
    tile_of = lambda a: a.reshape(ph // 8, 8, pw // 8, 8)
    fired_px = tile_of(r["fired"] & (kind == 1)).sum((1, 3))
    fired_edge = tile_of(r["fired"] & (kind == 2)).sum((1, 3))
    sky = tile_of(np.pad(f["depth"] == 1.0, ((0, ph - f["h"]), (0, pw - f["w"]))) | (kind == 2)).all((1, 3))
    t = r["tiles"]
    assert sky[0, 0] and t[0, 0] == 0
    assert not sky[0, 1] and t[0, 1] == 0                 # every lane has geometry, none fires: att == 0
    assert t[0, 2] == 1 and t[0, 3] == 64 and t[0, 6] == 64
    only = (fired_px == 0) & (fired_edge > 0)
    assert only.sum() >= 6 and only[0, 7] and only[5, 0]
    occ_t, lit_t = tile_of(r["occ"]).sum((1, 3)), tile_of(r["fired"] & ~r["occ"]).sum((1, 3))
    assert ((occ_t > 0) & (lit_t > 0) & only).sum() >= 6, "edge-only tiles with a mix of lit and occluded edge threads"
    # a tile whose firing lanes are ALL occluded (a warm cache answers every lane: the walk is skipped), in every group the cache test uses
    for gi in (0, 1, 2):
        gg, _, fr = references("shadows")[gi]
        ff, rr = fr[0]
        k2 = tc.thread_kind(ff["w"], ff["h"])
        p2h = ((k2.shape[0] + 7) // 8) * 8
        o2 = np.zeros((p2h, k2.shape[1]), np.int64); o2[: k2.shape[0]] = rr["occ"]
        occ2 = o2.reshape(p2h // 8, 8, k2.shape[1] // 8, 8).sum((1, 3))
        assert ((occ2 == rr["tiles"]) & (rr["tiles"] > 0)).any(), gg["name"]
    # no ray at all: the straight-up light; few: light (1,0,0) against the code-(0,0) normals
    frames = {f["name"]: r for _, f, r in all_frames("shadows")}
    assert frames["axis_light_up"]["count"] == 0 and not frames["axis_light_up"]["mask"].any()
    assert 0 < frames["axis_light_x"]["count"] < 200


@pytest.mark.parametrize("which", ("shadows", "ao"))
def test_edge_threads_fire_and_take_both_values(oracle, which):
    for g, f, r in all_frames(which):
        if f.get("no_rays"):
            continue
        edge = tc.thread_kind(f["w"], f["h"]) == 2
        fired, occ = r["fired"][..., edge], r["occ"][..., edge]
        if f["name"] in ("axis", "interval", "ao_main_L7", "ao_main_L25"):
            assert occ.any() and (fired & ~occ).any(), f"{f['name']}: edge-thread bits take one value only"


def test_fire_decisions_at_their_ties(oracle):
    frames = {f["name"]: (f, r) for _, f, r in all_frames("shadows")}
    f, r = frames["axis"]
    fired = r["fired"]
    codes = f["gb2"][0:8, 32:40, 0:2].view(np.float16).astype(np.float32)
    want = (1.0 - np.abs(codes[..., 0]) - np.abs(codes[..., 1])) > 0        # N.z > 0 against Wi = (0,0,1)
    assert np.array_equal(fired[0:8, 32:40], want) and want.any() and (~want).any()
    d = f["depth"][0:8, 40:48]
    assert np.array_equal(fired[0:8, 40:48], d != 1.0) and (d == 1.0).sum() >= 8
    # the light exactly at a pixel's P: no ray there, and none from its level (N.Wi == 0); at its ray origin: a ray of length bias
    f, r = frames["point_at_P"]
    assert not r["fired"][f.of("light_at_P")].any()
    level = np.pad(f["depth"] == 0.25, ((0, 3), (0, 4)))
    assert not r["fired"][level].any() and r["fired"][~level & (tc.thread_kind(f["w"], f["h"]) == 1)].any()
    f, r = frames["point_at_origin"]
    sel = f.of("light_at_origin")
    assert r["fired"][sel].all() and (r["rays"][sel][:, 3] == 0.5).all() and np.array_equal(r["rays"][sel][0, 4:7], np.float32([0, 0, 1]))
    # the cone: at the cosine no ray, one ulp inside one
    for k, want in ((0, False), (1, False), (-1, True)):
        f, r = frames[f"spot_outer{k:+d}"]
        assert bool(r["fired"][f["cone_pixel"]]) == want, (k, want)
        f, r = frames[f"spot_inner{k:+d}"]
        assert r["fired"][tc.thread_kind(f["w"], f["h"]) == 1].all()


def test_grazers_run_in_box_planes(oracle):
    from hybrid_rendering_amd import api
    g, f, r = [x for x in all_frames("shadows") if x[1]["name"] == "grazers"][0]
    boxes = api.bvh_child_boxes(g["tris"])
    planes = np.unique(np.concatenate([boxes["lo"][:, 2], boxes["hi"][:, 2]]))
    z = r["rays"][f.of("graze_plane")][:, 2]
    assert len(z) > 200 and np.isin(z, planes).all()
    # the edge row: y AND z on planes of ONE box that lies ahead of or around the origin; its neighbours one quantisation step beside in z
    e = r["rays"][f.of("graze_edge")]
    assert len(e) >= 12 and (np.unique(e[:, 1]).size == 1)
    for ray in e:
        on = ((boxes["lo"][:, 1] == ray[1]) | (boxes["hi"][:, 1] == ray[1])) & ((boxes["lo"][:, 2] == ray[2]) | (boxes["hi"][:, 2] == ray[2])) & (boxes["hi"][:, 0] > ray[0])
        assert on.any(), ray
    s = r["rays"][f.of("graze_edge_step")]
    assert len(s) >= 12 and (s[:, 1] == e[0, 1]).all()
    for ray in s:
        on = ((boxes["lo"][:, 1] == ray[1]) | (boxes["hi"][:, 1] == ray[1])) & (boxes["hi"][:, 0] > ray[0])
        dz = np.minimum(np.abs(boxes["lo"][on, 2] - ray[2]), np.abs(boxes["hi"][on, 2] - ray[2]))
        assert (np.abs(dz - boxes["step"][on, 2]) <= np.spacing(np.float32(16))).any(), ray
    zu = r["rays"][f.of("graze_ulps")][:, 2]
    assert len(zu) > 600 and not np.isin(zu, planes).all()
    assert (r["rays"][r["fired"]][:, 4:7] == np.float32([1, 0, 0])).all() and 0.1 < r["occ"][r["fired"]].mean() < 0.9


def test_ao_aim(oracle):
    """origins on the table's cell faces and one ulp beside them, outside the scene's box on all six sides, exactly at hi.z; the far scenes
    are where they say"""
    frames = {f["name"]: (g, f, r) for g, f, r in all_frames("ao")}
    g, f, r = frames["ao_main_L7"]
    lo, hi = g["tris"].reshape(-1, 3).min(0), g["tris"].reshape(-1, 3).max(0)
    assert np.array_equal(lo, g["box"][0]) and np.array_equal(hi, g["box"][1]) and hi[2] == tc.AO_BOX_HI[2]
    c, n = tc.host_cell(lo, hi, 7.0)
    assert c == np.float32(3.5) and g["cell"] == 3.5
    o = r["rays"][0]
    z = o[f.of("cell_face")][:, 2]
    k = np.round((z.astype(np.float64) - 0.5) / 3.5)
    face = (np.float32(0.5) + k.astype(np.float32) * np.float32(3.5)).astype(np.float32)
    assert ((z == face).sum() >= 10) and ((z == np.nextafter(face, np.float32(99))).sum() >= 10) and ((z == np.nextafter(face, np.float32(-99))).sum() >= 10)
    assert (o[f.of("below_lo")][:, 2] < lo[2]).all() and (o[f.of("above_hi")][:, 2] > hi[2]).all() and (o[f.of("at_hi")][:, 2] == hi[2]).all()
    # an origin exactly at hi on all three axes, in the table's last cell on z (hi.z == lo.z + 4 c), and a row / a column at hi.y / hi.x
    cy, cx = tc.AO_CORNER
    assert f.label(cy, cx) == "at_hi_corner" and np.array_equal(o[cy, cx, 0:3], hi) and hi[2] == np.float32(lo[2] + np.float32(4) * c) and n[2] == 5
    assert (o[cy, :f["w"], 1] == hi[1]).all() and (o[:f["h"], cx, 0] == hi[0]).all()
    px = tc.thread_kind(f["w"], f["h"]) > 0
    for a in (0, 1):
        assert (o[px][:, a] < lo[a]).sum() >= 40 and (o[px][:, a] > hi[a]).sum() >= 40
    g, f, r = frames["ao_planar"]
    assert np.ptp(g["tris"][..., 2]) == 0
    for where, T in tc.FAR_OFFSETS.items():
        g, f, r = frames[f"ao_far_{where}_L0.1"]
        p = g["tris"].reshape(-1, 3)
        assert np.abs(p.mean(0, dtype=np.float64) - np.asarray(T) - (0, 0, 4)).max() < 2 and np.ptp(p, 0).max() < 16
    assert g["tris"].reshape(-1, 3).min() < 8192 < g["tris"].reshape(-1, 3).max()


def test_far_scenes_are_aimed_at_the_entry_table(oracle):
    """ao_far_aimed_group: the aimed sample ray runs along +-z to 1e-6 in the cosine, its origin's z is on a face fl(lo.z + i c) of the host's
    table for the thread's ray_length or one ulp beside it, the thread's occluder is flat in z and the verdict flips between the occluder
    ending one ulp inside the axial reach (occluded) and one ulp beyond it (lit)"""
    for g, osc, frames in references("ao"):
        if not g["name"].startswith("ao_aimed"):
            continue
        lo, hi = g["box"]
        p = g["tris"].reshape(-1, 3)
        assert np.array_equal(p.min(0), lo) and np.array_equal(p.max(0), hi)
        flat = g["tris"][2:]
        assert (flat[:, :, 2].min(1) == flat[:, :, 2].max(1)).all() and g["n_aimed"] == len(g["tris"]) - 2 - g["background"] > 100
        q = np.spacing(np.float32(np.abs(hi).max()))
        for l, ((f, r), L) in enumerate(zip(frames, tc.FAR_LENGTHS)):
            c, n = tc.host_cell(lo, hi, L)
            assert float(c) == g["cells"][l] and f["ray_length"] == L
            sel = f.of(f"aimed_{L:g}")
            yy, xx = np.nonzero(sel)
            s = f["sample"][yy, xx]
            ray = r["rays"][s, yy, xx]
            assert len(ray) >= (100, 12)[l] and (np.abs(ray[:, 6]) > 1 - 1e-6).mean() > 0.9 and (ray[:, 6] > 0).any() and (ray[:, 6] < 0).any()
            i = np.round((ray[:, 2].astype(np.float64) - lo[2]) / float(c)).astype(np.float32)
            face = (lo[2] + i * c).astype(np.float32)
            k = f["ulps"][yy, xx]
            assert np.array_equal(ray[:, 2], tc.rc.step_ulps(face, k)) and all((k == v).sum() >= 3 for v in (-1, 0, 1))
            assert (i >= 1).all() and (i < n[2] - 1).all()
            occ, j = r["occ"][s, yy, xx], f["aim_j"][yy, xx]
            axial = np.abs(ray[:, 6]) > 1 - 1e-6
            assert occ[axial & (j >= 2)].all() and not occ[axial & (j <= -2)].any()
            assert 0.25 <= occ.mean() <= 0.75 and q >= 4e-4
            # sparse: no other aimed thread's occluder inside this thread's cell box (cell + ray_length + slack to every side)
            o = ray[:, 0:3].astype(np.float64)
            aimed = g["tris"][2:2 + g["n_aimed"]].astype(np.float64)
            lo_b, hi_b = aimed.min(1), aimed.max(1)
            half = float(c) + 1.01 * L
            inside = ((lo_b[None] <= o[:, None] + half) & (hi_b[None] >= o[:, None] - half)).all(2).sum(1)
            assert (inside <= 1).all(), inside.max()


@pytest.mark.parametrize("which", ("shadows", "ao"))
def test_the_oracle_passes_equal_packed_brute_force(oracle, which):
    """orc_shadows_ray_trace / orc_ao_ray_trace (which walk the oracle's BVH from G-buffers) against brute force over the generated rays:
    mask words (edge-thread bits included) and ray counts"""
    sob, sr = synth.blue_noise_tables()
    total = 0
    for g, osc, frames in references(which):
        for f, r in frames:
            if which == "shadows":
                mask, n = oracle.shadows_ray_trace(osc, f["ubo"], f["depth"], f["gb2"], sob, sr, f["bias"], 0)
            else:
                mask, n = oracle.ao_ray_trace(osc, f["ubo"], f["depth"], f["gb2"], sob, sr, f["bias"], f["ray_length"], 0, f["spp"])
            assert n == r["count"], (f["name"], n, r["count"])
            assert np.array_equal(mask, r["mask"]), f"{f['name']}: {int((mask != r['mask']).sum())} mask words differ from brute force"
            total += r["count"]
            print(f"{f['name']}: {r['count']} rays, {int(r['occ'].sum())} occluded")
    assert total > 20000


def test_pack_mask_inverts_unpack_mask():
    import helpers
    rng = np.random.RandomState(0)
    for w, h in tc.SIZES:
        ph, pw = tc.padded(w, h)
        bits = rng.randint(0, 2, (ph, pw)).astype(bool)
        m = tc.pack_mask(bits)
        assert m.shape == ((h + 3) // 4, (w + 7) // 8) and np.array_equal(helpers.unpack_mask(m, w, h), bits[:h, :w].astype(np.uint8))
        assert tc.tile_counts(bits).sum() == bits.sum() and tc.tile_counts(bits).shape == ((h + 7) // 8, pw // 8)


def test_cache_scenes_keep_the_count_and_move_by_ulps(oracle):
    g = tc.built("shadows")[0]
    b, c = tc.cache_scenes(g)
    assert b.shape == g["tris"].shape and len(c) < len(b)
    moved = (b != g["tris"]).any((1, 2))
    assert moved[: len(b) - g["background"]].mean() > 0.8 and not moved[len(b) - g["background"]:].any()
    assert np.abs(b.astype(np.float64) - g["tris"]).max() < 1e-4
