"""tests/emission_cases.py validated against tests/emission_reference.py and the oracle, without a GPU: the GPU tests are only as good as their
inputs.  Hits come from the oracle's closest-hit walk over the flattened world."""
import numpy as np
import pytest

import emission_cases as ec
import emission_reference as er

F = np.float32


@pytest.fixture(scope="module")
def world(oracle):
    isd = ec.instanced()
    flat = isd.flatten()
    r = ec.rays()
    tuv, prim = oracle.Scene(flat).closest_hit(r)
    return dict(isd=isd, flat=flat, rays=r, tuv=np.asarray(tuv, F), prim=np.asarray(prim, np.int32))


def test_the_world_is_small_and_the_three_kinds_number_it_alike(world):
    isd, flat = world["isd"], world["flat"]
    assert 90 <= flat.n_tris <= 130 and len(isd.materials) == ec.N_MATERIALS
    first, base, ids, n = isd.layout()
    assert int(first[-1] + n[-1]) == flat.n_tris and tuple(sorted(set(int(i) for i in ids))) == ec.MESH_IDS
    # the flat scene's attribute arrays are the meshes' arrays in instance order: the reference through attribute_index sees the same numbers
    ma = isd.mesh_arrays()
    q = ec.attribute_index(isd, np.arange(flat.n_tris))
    assert np.array_equal(ma["material"][q], flat.tri_material) and np.array_equal(ma["uvs"][q], flat.uvs)
    assert np.array_equal(ec.attribute_index(isd, np.array([-1, 0])), [-1, 0])
    # every mesh id but the room's has one material
    for mid in ec.MESH_IDS[1:]:
        assert len(set(flat.tri_material[flat.tri_mesh_id == mid])) == 1


@pytest.mark.parametrize("case", ["constant", "textured"])
def test_every_case_has_emitting_dark_and_missing_hits(world, case):
    isd, prim, tuv = world["isd"], world["prim"], world["tuv"]
    rgb, tex = ec.emissive_rgb(isd), (ec.EMISSIVE_TEX if case == "textured" else ec.NO_TEX)
    E, on = ec.expected(isd, rgb, tex, 1.0, prim, tuv)
    miss, hit = prim < 0, prim >= 0
    assert 100 < miss.sum() < len(prim) // 2, "misses"
    assert (hit & on).sum() > 200 and (hit & ~on).sum() > 1000, "hits on emitting and on dark materials"
    mat = world["flat"].tri_material[np.maximum(prim, 0)]
    assert (hit & (mat == ec.EMITTER)).sum() > 50 and (hit & (mat == ec.QUAD)).sum() > 50, "both emitters are hit"
    assert np.all(E[~on] == 0) and np.all((E[on] != 0).any(1) | (mat[on] == ec.QUAD)), "dark and missing hits give 0"
    e = E[hit & (mat == ec.EMITTER)]
    assert np.all(e == rgb[ec.EMITTER]), "scale 1: the constant itself"
    E37, _ = ec.expected(isd, rgb, tex, 3.7, prim, tuv)
    assert np.array_equal(E37, (F(3.7) * E).astype(F)) and E37.dtype == np.float32


def test_the_textured_case_wraps_in_all_four_quadrants_and_has_weights_of_zero_and_one(world):
    isd, prim, tuv = world["isd"], world["prim"], world["tuv"]
    ma = isd.mesh_arrays()
    q = ec.attribute_index(isd, prim)
    on_quad = (q >= 0) & (ma["material"][np.maximum(q, 0)] == ec.QUAD)
    tu, tv = er.hit_uv(ma["uvs"], q[on_quad], tuv[on_quad, 1], tuv[on_quad, 2])
    for sx in (-1, 1):
        for sy in (-1, 1):
            assert ((np.sign(tu) == sx) & (np.sign(tv) == sy)).sum() >= 5, (sx, sy)
    assert (tu > 1).any() and (tv > 1).any() and (tu < -1).any() and (tv < -1).any(), "REPEAT both ways, more than once around"
    # the crafted hits: vertex 0 of the quad's first triangle sits on a texel centre
    cprim, ctuv = ec.crafted_hits(isd)
    cq = ec.attribute_index(isd, cprim)
    ctu, ctv = er.hit_uv(ma["uvs"], cq[:3], ctuv[:3, 1], ctuv[:3, 2])
    rgbs, fx, fy = er.sample_rgb(isd.textures[ec.TEX_EMISSIVE], ctu, ctv)
    assert fx[0] == 0 and fy[0] == 0 and (ctu[0], ctv[0]) == (F(0.125), F(0.375)), "bilinear weights of exactly 1 and 0"
    assert np.array_equal(rgbs[0], isd.textures[ec.TEX_EMISSIVE][1, 0, :3].astype(F) / F(255.0)), "... which return the texel itself"
    E, on = ec.expected(isd, ec.emissive_rgb(isd), ec.EMISSIVE_TEX, 1.0, cprim, ctuv)
    assert on[:-1].all() and not on[-1] and np.all(E[-1] == 0)
    # the texture replaces the constant; without it the quad's constant comes back
    E0, _ = ec.expected(isd, ec.emissive_rgb(isd), ec.NO_TEX, 1.0, cprim, ctuv)
    assert np.all(E0[0] == ec.emissive_rgb(isd)[ec.QUAD]) and not np.array_equal(E0[0], E[0])


def test_the_select_rule():
    rgb = np.array([[0, 0, 0], [0, 0.5, 0], [0, 0, 0], [-0.0, 0, 0]], F)
    assert list(er.emits(rgb, [-1, -1, 2, -1])) == [False, True, True, False]


def test_helpers_make_the_scenes_the_gpu_tests_compare(world):
    isd = world["isd"]
    w = ec.without_material(isd, ec.EMITTER)
    assert w.flatten().n_tris == world["flat"].n_tris - 1 and ec.EMITTER not in set(w.flatten().tri_material)
    h = ec.with_hidden_material(isd, ec.EMITTER)
    assert h.material_textures[ec.EMITTER, 0] == ec.TEX_HOLE and np.all(h.textures[ec.TEX_HOLE][..., 3] == 0)
    b = ec.black(isd)
    assert np.all(b.materials[:, :4] == 0) and np.array_equal(b.materials[:, 5:], isd.materials[:, 5:]) and np.all(b.material_textures[:, :4] == -1)
    rgb, table = ec.per_mesh_id_rgb()
    flat = world["flat"]
    for mid, c in table.items():
        assert np.all(rgb[flat.tri_material[flat.tri_mesh_id == mid]] == c), mid


def test_the_oracle_alone_keeps_the_lit_reflections_under_the_clamp(oracle, world):
    """the condition of the GPU additivity test: the ORACLE's reflections trace image of the emission-free world under ec.light() has at most 10 % of
    its traced texels at the 0.7 clamp"""
    from hybrid_rendering_amd import synth, synth_env
    from oracle import pyoracle_ddgi as od, pyoracle_reflections as orf
    W, H = ec.REFL_W, ec.REFL_H
    isd = ec.instanced(emissive=False)
    osc = oracle.InstancedScene(isd)
    ubo = synth.make_ubo(ec.camera(W / H), None, ec.light())
    cur = ec.all_mirrors(osc.gbuffer(ubo, W, H))
    grid = ec.ddgi_grid()
    sky = synth_env.sky_cubemap(16)
    env = dict(sky=sky, prefiltered=synth_env.prefiltered_chain(sky, 5), pre_size=16, pre_levels=5, lut=synth_env.brdf_lut(16))
    sob, sr = synth.blue_noise_tables()
    odd = od.DDGIPass(grid, infinite_bounces=False)
    odd.render(osc, ubo, cur, sky, synth_env.random_orientation(np.random.RandomState(4)), 0)
    irr, dep = odd.current_read()
    orr = orf.ReflectionsPass(W, H)
    orr.render(osc, ubo, grid, cur, cur, sob, sr, 0, env, irr, dep, ping_pong=False)
    trace = orr.stages["trace"]
    traced = cur["depth"] != 1.0
    assert traced.sum() > 0.9 * W * H and orr.stages["rays"] >= traced.sum()
    clamp = np.float16(0.7).view(np.uint16)
    at_clamp = (trace[..., :3] == clamp).any(-1) & traced
    share = at_clamp.sum() / traced.sum()
    print(f"traced texels {traced.sum()}, at the 0.7 clamp {at_clamp.sum()} ({100 * share:.2f} %)")
    assert share <= 0.10
    lit = (trace[..., :3].view(np.float16)[traced] > 0).any(-1).mean()
    assert lit > 0.5, "the light reaches what the mirrors see"


def test_the_cameras_see_what_the_gpu_tests_need(oracle, world):
    """61 x 37 from inside: every mesh id, the one-triangle emitter and the quad each with 2 x 2 pixel blocks inside them (what the ground-truth check uses:
    a jittered ray of pixel (x, y) passes between the centres of (x, y) .. (x + 1, y + 1)); from outside: sky and room"""
    from hybrid_rendering_amd import synth
    W, H = 61, 37
    osc = oracle.InstancedScene(world["isd"])
    g = osc.gbuffer(synth.make_ubo(ec.camera(W / H), None, ec.light()), W, H)
    ids = g["gb3"][..., 2].view(np.float16).astype(np.int32)
    assert (g["depth"] != 1.0).all() and set(np.unique(ids)) == set(ec.MESH_IDS)
    for mid in (4, 5):
        m = ids == mid
        assert (m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]).sum() >= 3, mid
    g = osc.gbuffer(synth.make_ubo(ec.camera_outside(W / H), None, ec.light()), W, H)
    sky = g["depth"] == 1.0
    assert 0.2 < sky.mean() < 0.9
