"""The shadow and AO TRACE LAUNCHES (k_shadows_trace, k_ao_trace, their two-level twins, k_ao_entry_grid) against BRUTE FORCE on the
adversarial G-buffers of tests/trace_cases.py: fire / no-fire ties, tile shapes (all sky, att == 0, one lane, full, only edge threads),
edge threads of ragged images whose rays hit, rays exactly through vertices, shared edges and fan hubs and 1 .. 8 ulps beside them, hits at
t_min / t_max +- ulps, rays in the face planes of the child boxes, the occluder cache (cold, warm, after the geometry moved by ulps, with
stale indices) and the AO entry-node table (origins on cell faces, outside the table, after a change of ray_length or scene on a live
pass, small scenes at coordinates 5000 / 8190 / 50000 — dense ones, and sparse ones AIMED at the table's cell boxes: origins on cell faces,
a sample ray along the axis, a flat occluder within ulps of the axial reach).

Reference: the oracle's any_hit(brute_force=True) — no box test of any kind — over the exact ray of every thread, which the oracle's ray
generation reproduces bit for bit (tests/test_trace_cases.py pins the reference and keeps these tests from passing vacuously).
Compared: every mask word (edge-thread bits included), ray_count() and the per-tile ray counts.  Mismatches allowed: 0.  ray_trace() only.
The closest-hit launches (k_ddgi_trace, k_refl_trace) are pinned the same way by tests/closest_cases.py and tests/test_gpu_closest_edges.py.

That the tests bite (docs/EXPERIMENTS.md, "Adversarial G-buffers"): four throw-away variants of the library, each with ONE answer-changing
mutation, were run against this file alone — the entry table built without its grow, the cached-triangle test with 10000 for t_max,
`att >= 0`, trace_lane_kind without edge threads; each fails tests here.  A fifth, the table's cells grown by 0.99 ray_length, fails the
aimed far family and nothing else."""
import numpy as np
import pytest

import helpers
import trace_cases as tc
from test_gpu_ray_edges import BUILDS, hexrow, set_build_env
from test_trace_cases import reference, references

pytestmark = pytest.mark.gpu

KIND = {0: "no thread", 1: "pixel", 2: "edge thread"}


def unpack_padded(mask):
    mh, mw = mask.shape[-2:]
    bits = np.zeros(mask.shape[:-2] + (mh * 4, mw * 8), bool)
    for ly in range(4):
        for lx in range(8):
            bits[..., ly::4, lx::8] = ((mask >> np.uint32(ly * 8 + lx)) & 1) != 0
    return bits


class Rig:
    """blue-noise tables and G-buffers on the device, one pass object per (kind, size)"""

    def __init__(self, hr, ctx):
        import torch
        from hybrid_rendering_amd import synth
        self.hr, self.ctx, self.torch = hr, ctx, torch
        sob, sr = synth.blue_noise_tables()
        self.sob, self.sr = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()

    def inputs(self, f):
        gb = helpers.to_cuda(dict(depth=f["depth"], gb2=f["gb2"], gb3=np.zeros_like(f["gb2"])))
        return self.hr.frame_inputs(gb, gb, f["ubo"], 0, 0, self.sob, self.sr)

    def shadows(self, p, gsc, f):
        p.params.bias = f["bias"]
        p.ray_trace(gsc, self.inputs(f))
        self.torch.cuda.synchronize()
        return p.image(p.IMG_MASK).cpu().numpy().view(np.uint32).copy(), int(p.ray_count()), p.tile_ray_counts().astype(np.int64)

    def ao(self, p, gsc, f):
        p.params.bias, p.params.ray_length, p.params.spp = f["bias"], f["ray_length"], f["spp"]
        p.ray_trace(gsc, self.inputs(f))
        self.torch.cuda.synchronize()
        mh = (f["h"] + 3) // 4
        mask = p.image(p.IMG_MASK).cpu().numpy().view(np.uint32)[: f["spp"] * mh].reshape(f["spp"], mh, -1).copy()
        return mask, int(p.ray_count()), None


def compare(f, r, got, what):
    """0 differing mask words, equal ray counts; the message names pixel, family, thread kind and the ray"""
    mask, count, tiles = got
    assert mask.shape == r["mask"].shape, (what, mask.shape, r["mask"].shape)
    bad_words = int((mask != r["mask"]).sum())
    lines = []
    if bad_words:
        lit_ref, lit_got = r["fired"] & ~r["occ"], unpack_padded(mask)
        kind = tc.thread_kind(f["w"], f["h"])
        diff = np.argwhere(lit_ref != lit_got)
        per_family = {}
        for idx in diff:
            y, x = int(idx[-2]), int(idx[-1])
            per_family[f.label(y, x)] = per_family.get(f.label(y, x), 0) + 1
        lines.append(f"  by family: {per_family}")
        for idx in diff[:8]:
            y, x = int(idx[-2]), int(idx[-1])
            ray = r["rays"][tuple(idx)]
            lines.append(f"  {'sample %d ' % idx[0] if len(idx) == 3 else ''}pixel ({x}, {y}) [{KIND[int(kind[y, x])]}], family {f.label(y, x)} ({int(f['ulps'][y, x]):+d}): "
                         f"lit ref {int(lit_ref[tuple(idx)])} got {int(lit_got[tuple(idx)])}; fired {int(ray[7])}; ray o, t_max, d = {hexrow(ray[:7])}")
    if count != r["count"]:
        lines.append(f"  ray_count() {count}, brute force fired {r['count']}")
    if tiles is not None and not np.array_equal(tiles, r["tiles"]):
        lines.append(f"  tile_ray_counts() differ in tiles {np.argwhere(tiles != r['tiles'])[:8].tolist()}: got {tiles[tiles != r['tiles']][:8].tolist()} want {r['tiles'][tiles != r['tiles']][:8].tolist()}")
    print(f"{what}: {r['count']} rays, {int(r['occ'].sum())} occluded; {bad_words} mask words differ")
    assert not lines, f"{what}: {bad_words} mask words differ from brute force\n" + "\n".join(lines)


@pytest.fixture(scope="module")
def rig(hr, ctx):
    return Rig(hr, ctx)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("group", range(4))
def test_shadow_frames_match_brute_force(oracle, hr, ctx, rig, monkeypatch, group, build):
    """every crafted shadow frame, per BVH build (default, spatial splits at 0.1, SAH depth 3): mask words, ray count, per-tile ray counts"""
    g, osc, frames = references("shadows")[group]        # before the build switches: the grazers aim at the default build's boxes
    set_build_env(monkeypatch, BUILDS[build])
    gsc = hr.Scene(ctx, tc.scene_data(g["tris"], g["name"]))
    p = hr.RayTracedShadows(ctx, frames[0][0]["w"], frames[0][0]["h"])
    try:
        for f, r in frames:
            compare(f, r, rig.shadows(p, gsc, f), f"{g['name']}/{f['name']}/{build}")
    finally:
        p.close(); gsc.close()


def stale_at_the_end(hr, ctx, oracle, gsc, tris, f):
    """A scene D with n_tri_refs == k, where BOTH k and k - 1 are indices a pass caches after tracing frame f on `gsc` (scene `tris`): pixels
    whose ray has one single-reference triangle as its only occluder cache that triangle's reference index; read_bvh() tells which.  On D the
    stale index k must be refused (k == n_tri_refs) and k - 1 names D's last reference."""
    _, refs = gsc.read_bvh()
    prim = refs[:, 12:16].copy().view(np.uint32).reshape(-1)       # TriGPU::prim (csrc/bvh.h)
    # the layout is what this reads it as: every reference names a triangle, and every triangle with an area is named (repeats: spatial splits)
    area = np.linalg.norm(np.cross(tris[:, 1].astype(np.float64) - tris[:, 0], tris[:, 2].astype(np.float64) - tris[:, 0]), axis=1)
    named = np.zeros(len(tris), bool)
    assert refs.shape[1] == 48 and int(prim.max()) < len(tris), "read_bvh(): not the TriGPU layout of csrc/bvh.h"
    named[prim] = True
    assert named[area > 0].all() and len(prim) >= int((area > 0).sum()), "read_bvh(): references do not cover the triangles"
    rays = tc.frame_rays(f)
    q = tc.query_rays(rays)
    osc = oracle.Scene(tc.scene_data(tris, "cache"))
    _, first = osc.closest_hit(q, brute_force=True)
    single = np.zeros(f["family"].shape, bool)
    for name in ("vertex", "edge", "backface"):                     # one triangle above the pixel and nothing else
        single |= f.of(name)
    cached_prims = np.unique(first.reshape(single.shape)[single & (first.reshape(single.shape) >= 0)])
    once = np.flatnonzero(np.bincount(prim, minlength=len(tris)) == 1)
    is_cached = np.isin(prim, np.intersect1d(cached_prims, once))
    ks = np.flatnonzero(is_cached[1:] & is_cached[:-1]) + 1         # k and k - 1 both cached
    assert len(ks) > 0, "no two neighbouring references are cached"
    for k in ks[::-1][:8]:
        n = int(k)
        for _ in range(4):                                          # spatial splits may add references: shrink until the count is k
            d = hr.Scene(ctx, tc.scene_data(tris[:n], "cache"))
            have = int(d.refresh_info().tri_bytes) // 48
            if have == k:
                return d, tris[:n], int(k)
            d.close()
            n -= have - int(k)
            if n <= 0:
                break
    raise AssertionError("no scene with a reference count at a cached index")


@pytest.mark.parametrize("group,axes", ((0, (0, 1)), (1, (2,)), (2, (2,))))
def test_occluder_cache_cold_warm_moved_and_stale(oracle, hr, ctx, rig, monkeypatch, group, axes):
    """ONE pass object: frame 0 cold; frame 1 the same inputs (every occluded lane is answered by its cached triangle, tiles whose lanes all
    are skip the walk); frame 2 a scene of as many triangles, each occluder moved by -8 .. 8 ulps (a cached triangle now just misses or just
    hits: at an edge or vertex in the axis group, at t_min / t_max in the interval group, at the point light's distance in the punctual
    group); frame 3 (axis group) a scene whose reference count k is itself a cached index, as is k - 1 (stale_at_the_end); then a scene with
    a random 60 % of the triangles (stale indices past the end, and naming other triangles); last the first scene again.  Every frame equals
    brute force over ITS scene and a pass created with HR_SHADOW_CACHE=0."""
    g, osc, frames = references("shadows")[group]
    f, r = frames[0]
    b, c = tc.cache_scenes(g, axes)
    scenes = [g["tris"], g["tris"], b, c, g["tris"]]
    gpu = {id(t): hr.Scene(ctx, tc.scene_data(t, "cache")) for t in (g["tris"], b, c)}
    if group == 0:
        d_scene, d, k = stale_at_the_end(hr, ctx, oracle, gpu[id(b)], b, f)
        print(f"{g['name']}: scene with n_tri_refs == {k}, both {k} and {k - 1} cached by the frame before")
        gpu[id(d)] = d_scene
        scenes.insert(3, d)
    refs = {id(g["tris"]): r}
    for t in scenes[2:-1]:
        refs[id(t)] = reference(oracle.Scene(tc.scene_data(t, "cache")), f)
        assert not np.array_equal(refs[id(t)]["mask"], r["mask"]), "a changed scene changes no bit"
    cached = hr.RayTracedShadows(ctx, f["w"], f["h"])
    monkeypatch.setenv("HR_SHADOW_CACHE", "0")
    plain = hr.RayTracedShadows(ctx, f["w"], f["h"])
    monkeypatch.delenv("HR_SHADOW_CACHE")
    try:
        for i, t in enumerate(scenes):
            got = rig.shadows(cached, gpu[id(t)], f)
            compare(f, refs[id(t)], got, f"{g['name']} cache frame {i}")
            ref = rig.shadows(plain, gpu[id(t)], f)
            compare(f, refs[id(t)], ref, f"{g['name']} cache frame {i}, HR_SHADOW_CACHE=0")
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
            if i == 1:      # the warm frame walks less than the cold one did: the instrumented kernel, cache on, against the full walk
                full, warm = cached.trace_stats(gpu[id(t)], rig.inputs(f)), cached.trace_stats(gpu[id(t)], rig.inputs(f), timed=True)
                print(f"{g['name']}: rays, nodes, triangles: full walk {full}, warm cache {warm}")
                assert warm[0] == full[0] == refs[id(t)]["count"] and warm[1] < full[1]
    finally:
        cached.close(); plain.close()
        for s in gpu.values():
            s.close()


def _ao_frames():
    """{frame name: (group, frame, reference)}"""
    return {f["name"]: (g, f, r) for g, _, fr in references("ao") for f, r in fr}


AO_SEQUENCE = ("ao_main_L7", "ao_main_L0.1", "ao_main_L25", "ao_main_L0.5",                 # ray_length 7 -> 0.1 -> 25 -> 0.5 on a live pass
               "ao_far_5000_L0.1", "ao_far_5000_L0.5",                                         # a scene swap, far from the origin
               "ao_far_50000_L0.5", "ao_far_50000_L0.1", "ao_far_8190_L0.1", "ao_far_8190_L0.5",
               "ao_main_L0.5", "ao_main_L7")                                                   # and back


def _run_ao(hr, ctx, rig, names, what):
    fr = _ao_frames()
    scenes, p = {}, None
    try:
        for i, n in enumerate(names):
            g, f, r = fr[n]
            if g["name"] not in scenes:
                scenes[g["name"]] = hr.Scene(ctx, tc.scene_data(g["tris"], g["name"]))
            if p is None:
                p = hr.RayTracedAO(ctx, f["w"], f["h"], 0)
            compare(f, r, rig.ao(p, scenes[g["name"]], f), f"{what} step {i}: {n}")
    finally:
        if p is not None:
            p.close()
        for s in scenes.values():
            s.close()


def test_ao_live_pass_matches_brute_force(oracle, hr, ctx, rig):
    """ONE pass object, 4 spp: every sample plane and ray_count() while ray_length and the scene change under the entry-node table"""
    _run_ao(hr, ctx, rig, AO_SEQUENCE, "ao")


def test_ao_one_sample_and_a_planar_scene(oracle, hr, ctx, rig):
    _run_ao(hr, ctx, rig, ("ao_main_spp1", "ao_main_L0.1"), "ao spp 1 then 4")
    _run_ao(hr, ctx, rig, ("ao_planar", "ao_planar_spp1"), "ao planar")


def test_ao_without_the_entry_table(oracle, hr, ctx, rig, monkeypatch):
    """HR_AO_ENTRY_GRID=0: every pixel finds its entry node by the descent"""
    monkeypatch.setenv("HR_AO_ENTRY_GRID", "0")
    _run_ao(hr, ctx, rig, ("ao_main_L7", "ao_main_L0.1", "ao_far_50000_L0.1", "ao_far_5000_L0.5", "ao_far_8190_L0.1"), "ao, HR_AO_ENTRY_GRID=0")


AIMED = tuple(f"ao_aimed_{where}_L{L:g}" for where in tc.FAR_OFFSETS for L in tc.FAR_LENGTHS)


@pytest.mark.parametrize("grid", ("table", "descent"))
def test_ao_far_scenes_aimed_at_the_entry_table(oracle, hr, ctx, rig, monkeypatch, grid):
    """Scenes at 5000 / 50000 / 8190 whose origins sit on the faces of the entry table's cells (and one ulp beside them), whose aimed sample
    runs along +-z and whose only occluder is a flat triangle ending 0 .. 3 ulps inside / 1 .. 2 ulps beyond the axial reach: the case a
    cell box with too little slack loses.  With the table and with the per-pixel descent (HR_AO_ENTRY_GRID=0)."""
    if grid == "descent":
        monkeypatch.setenv("HR_AO_ENTRY_GRID", "0")
    _run_ao(hr, ctx, rig, AIMED, f"ao aimed, {grid}")


def _two_meshes(g):
    """the group as a shared instanced scene: occluders and background as two meshes under identity matrices (object space == world space)"""
    from hybrid_rendering_amd import synth
    n_fg = len(g["tris"]) - g["background"]
    meshes = [tc.scene_data(g["tris"][:n_fg], "occluders"), tc.scene_data(g["tris"][n_fg:], "background")]
    return synth.InstancedSceneData(meshes=meshes, instances=[(synth.model_matrix(), 0, 1), (synth.model_matrix(), 1, 2)], materials=meshes[0].materials, name=g["name"] + "_two_level")


def test_two_level_kernels_match_brute_force(oracle, hr, ctx, rig):
    """k_shadows_trace<SHARED> and k_ao_trace<SHARED> on hr.InstancedScene(shared=True) with enable_two_level_passes(): the axis-light
    frames and the AO frames at ray_length 7 and 0.1"""
    gs, _, sframes = references("shadows")[0]
    ga, _, aframes = references("ao")[0]
    for g in (gs, ga):
        isd = _two_meshes(g)
        assert np.array_equal(isd.flatten().verts.view(np.uint32), g["tris"].view(np.uint32)), "identity instances move a vertex"
    s1, s2 = hr.InstancedScene(ctx, _two_meshes(gs), shared=True).enable_two_level_passes(), hr.InstancedScene(ctx, _two_meshes(ga), shared=True).enable_two_level_passes()
    ps, pa = hr.RayTracedShadows(ctx, *tc.SIZES[0]), hr.RayTracedAO(ctx, *tc.SIZES[0], 0)
    try:
        for f, r in sframes:
            compare(f, r, rig.shadows(ps, s1, f), f"two-level shadows/{f['name']}")
        for f, r in aframes[:2]:
            compare(f, r, rig.ao(pa, s2, f), f"two-level ao/{f['name']}")
    finally:
        ps.close(); pa.close(); s1.close(); s2.close()
