"""hr_env on the device (csrc/env.hip) against the float32 numpy restatement of its contract (tests/env_reference.py; include/hr_env.h,
DESIGN.md §3.5), bit for bit: the sky copy, the GGX-prefiltered chain, SH9 and the split-sum LUT, on the smallest shapes that reach every
branch; then the object's state, graph capture, what the consumers' own fetch functions read from its storage, and the composite's SH9 binding.
The reference is fed the library's own sample table (tests/test_env_host.py holds that table to numpy's)."""
import ctypes as C

import numpy as np
import pytest

import env_reference as er
import helpers
import shading_cases as sc
from hybrid_rendering_amd import synth, synth_env

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def env(hr):
    from hybrid_rendering_amd import env as envmod
    return envmod


def _sky(name):
    if name == "a":
        return synth_env.sky_cubemap(size=8)
    if name == "b":
        return synth_env.sky_cubemap(size=8, sun_dir=(-0.5, 0.4, -0.7), intensity=2.5)
    if name == "a16":
        return synth_env.sky_cubemap(size=16)
    assert name == "extreme"
    # one texel at the top of fp16 (sums and quotients near it overflow, or do not, as the contract's operations say) and one exact zero row
    sky = synth_env.sky_cubemap(size=8).copy()
    sky.view(np.float16)[2, 3, 5, :3] = 65504.0
    sky[4, 6, :, :3] = 0
    return sky


def _reference(env, sky_name, P, levels, lut, n):
    """computed once per shape and never modified"""
    key = (sky_name, P, levels, lut, n)
    if key not in _REF:
        sky, table = _sky(sky_name), env.sample_table(n)
        r = dict(sky=sky, chain=er.prefiltered_chain(sky, P, levels, table), lut=er.brdf_lut(lut, table), sh9=er.sh9(sky).view(np.uint32))
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _f16(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda().view(torch.float16)      # np.array: a writable copy (the shared references are read-only)


def _read(E):
    import torch
    torch.cuda.synchronize()
    return dict(sky=helpers.bits16(E.sky()), chain=helpers.bits16(E.prefiltered()), lut=helpers.bits16(E.brdf_lut()), sh9=E.read_sh9().view(np.uint32))


def _assert_equal(got, ref, what):
    for k in ("sky", "chain", "lut", "sh9"):
        helpers.assert_bits_equal_nan(got[k], np.asarray(ref[k]), f"{what}: {k}")


@pytest.mark.parametrize("sky_name, sky_size, n", [("a", 8, 64), ("a", 8, 192), ("a16", 16, 64), ("extreme", 8, 64)],
                         ids=["n64", "n192", "sky16_fetch", "fp16_max_and_zero_row"])
def test_env_matches_the_contract_bit_for_bit(hr, ctx, env, sky_name, sky_size, n):
    """prefiltered 8 with 4 levels (8, 4, 2, 1: the 1 x 1 level puts N on the axes, so +-Z take the |N.z| >= 0.999 frame); 64 samples = one per
    lane, 192 = three per lane and no power of two; sky 16 over a chain of 8: level 0 is a fetch, not a copy"""
    P, levels, lut = 8, 4, 8
    ref = _reference(env, sky_name, P, levels, lut, n)
    E = env.Environment(ctx, sky_size=sky_size, prefiltered_size=P, prefiltered_levels=levels, brdf_lut_size=lut, n_samples=n)
    before = _read(E)
    assert not before["sky"].any() and not before["chain"].any() and not before["sh9"].any()      # zeros until the first update
    helpers.assert_bits_equal_nan(before["lut"], np.asarray(ref["lut"]), "the LUT is integrated at creation")
    E.update(_f16(ref["sky"]))
    got = _read(E)
    _assert_equal(got, ref, f"{sky_name} n={n}")
    val = got["chain"].view(np.float16).astype(np.float32)
    if sky_name == "extreme":
        assert np.isinf(val).any() or (val == 65504.0).any()
        assert np.isfinite(got["sh9"].view(np.float32)).all()
    else:
        assert np.isfinite(val).all() and (val[:, 3] == 1.0).all() and len(np.unique(got["chain"][:, 0])) > 30
    if sky_size == P:
        assert np.array_equal(got["chain"][:6 * P * P], np.asarray(ref["sky"]).reshape(-1, 4))      # level 0: a bit copy
    E.close()


@pytest.mark.parametrize("lut", [1, 5])
def test_env_lut_of_odd_sizes(hr, ctx, env, lut):
    n = 64
    E = env.Environment(ctx, sky_size=8, prefiltered_size=8, prefiltered_levels=1, brdf_lut_size=lut, n_samples=n)
    got = _read(E)["lut"]
    assert got.shape == (lut, lut, 2)
    helpers.assert_bits_equal_nan(got, er.brdf_lut(lut, env.sample_table(n)), f"LUT of size {lut}")
    assert got.any()
    # a single level: roughness 0 is never integrated, the chain is level 0 alone
    sky = _sky("a")
    E.update(_f16(sky))
    assert np.array_equal(_read(E)["chain"], sky.reshape(-1, 4))
    E.close()


def _pointers(E):
    e = E.get()
    return (e.sky, e.sky_size, e.prefiltered, e.prefiltered_size, e.prefiltered_levels, e.brdf_lut, e.brdf_lut_size, E.sh9_device())


def test_env_state_across_updates(hr, ctx, env):
    """sky A, sky B, sky A again: the third result is the first; the LUT never changes; the pointers handed out never change"""
    P, levels, lut, n = 8, 4, 8, 64
    ra, rb = _reference(env, "a", P, levels, lut, n), _reference(env, "b", P, levels, lut, n)
    assert not np.array_equal(ra["chain"], rb["chain"]) and not np.array_equal(ra["sh9"], rb["sh9"])
    E = env.Environment(ctx, sky_size=8, prefiltered_size=P, prefiltered_levels=levels, brdf_lut_size=lut, n_samples=n)
    ptrs = _pointers(E)
    assert all(ptrs) and ptrs[1:2] + ptrs[3:5] + ptrs[6:7] == (8, P, levels, lut)
    a, b = _f16(ra["sky"]), _f16(rb["sky"])
    for which, ref in ((a, ra), (b, rb), (a, ra)):
        E.update(which)
        _assert_equal(_read(E), ref, "A, B, A")
        assert _pointers(E) == ptrs
    assert E.sky().data_ptr() != a.data_ptr()      # the env reads its own copy of the sky
    E.close()


def test_env_update_captured_into_a_graph(hr, ctx, env):
    """hr_env_update on one stream is a linear graph (a copy and four launches): a replay derives everything from what is in the caller's sky
    buffer THEN"""
    import torch
    P, levels, lut, n = 8, 4, 8, 64
    ra, rb = _reference(env, "a", P, levels, lut, n), _reference(env, "b", P, levels, lut, n)
    E = env.Environment(ctx, sky_size=8, prefiltered_size=P, prefiltered_levels=levels, brdf_lut_size=lut, n_samples=n)
    buf = _f16(ra["sky"])
    E.update(buf)
    _assert_equal(_read(E), ra, "eager")
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        E.update(buf)
    for name, ref in (("b", rb), ("a", ra), ("b", rb)):
        buf.copy_(_f16(ref["sky"]))
        torch.cuda.synchronize()
        graph.replay()
        _assert_equal(_read(E), ref, f"replay with sky {name}")
    E.close()


def _cube_inputs():
    """CUBE elements (csrc/selftest_shading.h: 0-2 d, 3 lod, 4-5 lut u, v): directions on every face, on face edges and corners and off them; lod on
    every level, on x.5 and past both ends; the LUT's corners, its row and column ends, and texel borders"""
    rng = np.random.RandomState(3)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    dirs = np.concatenate([axes, axes + np.float32(0.37) * axes[:, [1, 2, 0]] - np.float32(0.21) * axes[:, [2, 0, 1]], sc.cube_edge_dirs(), sc.cube_corner_dirs(),
                           sc.cube_neighbour_dirs()[0], sc.rand_unit(rng, 64)]).astype(np.float32)
    lods = np.array([0.0, 1.0, 2.0, 3.0, 0.5, 1.5, 2.5, 0.49, 2.51, -1.0, 3.5, 7.0], np.float32)
    uvs = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [0.999, 0.001], [0.001, 0.999], [0.125, 0.875], [0.5, 0.25], [0.26, 0.51], [-0.5, 2.0]], np.float32)
    e = sc.elems(len(dirs) * len(lods))
    e[:, 0:3] = np.repeat(dirs, len(lods), 0)
    e[:, 3] = np.tile(lods, len(dirs))
    e[:, 4:6] = uvs[np.arange(len(e)) % len(uvs)]
    return e


def test_consumers_read_what_env_wrote(hr, ctx, env):
    """CubeMap::fetch, prefiltered_fetch and lut_fetch (hr_selftest_shading's CUBE mode) over hr_env_get's pointers and over the reference's arrays
    uploaded by hand: the level offsets, the texel order and the LUT's row / column sense are the consumers'"""
    import torch
    from oracle import pyoracle as po
    P, levels, lut, n = 8, 4, 8, 64
    ref = _reference(env, "a", P, levels, lut, n)
    E = env.Environment(ctx, sky_size=8, prefiltered_size=P, prefiltered_levels=levels, brdf_lut_size=lut, n_samples=n)
    E.update(_f16(ref["sky"]))
    torch.cuda.synchronize()
    e = E.get()
    sizes = dict(cube_size=8, pre_size=P, pre_levels=levels, lut_size=lut)
    by_hand = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(ref[k])).view(np.uint8).reshape(-1).copy()).cuda() for k in ("sky", "chain", "lut")}
    dummy = np.zeros(1, np.uint8)      # shading_tables stores the address given, not the array's
    tabs = [po.shading_tables(dict(cube=dummy, prefiltered=dummy, lut=dummy, **sizes), address=dict(cube=e.sky, prefiltered=e.prefiltered, lut=e.brdf_lut)),
            po.shading_tables(dict(cube=dummy, prefiltered=dummy, lut=dummy, **sizes),
                              address=dict(cube=by_hand["sky"].data_ptr(), prefiltered=by_hand["chain"].data_ptr(), lut=by_hand["lut"].data_ptr()))]
    inp = _cube_inputs()
    x = torch.from_numpy(inp).cuda()
    outs = []
    for tab in tabs:
        out = torch.full((8, len(inp)), 7.0, dtype=torch.float32, device="cuda")
        st = hr.lib().hr_selftest_shading(C.c_int32(sc.CUBE), C.c_int64(len(inp)), C.c_void_p(x.data_ptr()), C.c_void_p(C.addressof(tab)), C.c_int32(8),
                                          C.c_void_p(out.data_ptr()), None)
        assert st == 0, hr.lib().hr_last_error()
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    helpers.assert_bits_equal_nan(outs[0].view(np.uint32), outs[1].view(np.uint32), "CUBE mode over hr_env_get's pointers against the reference's arrays")
    # the elements do tell levels and LUT texels apart: the prefiltered fetch of one direction differs between lods, the LUT planes take many values
    pre = outs[0][3:6].T.reshape(-1, 12, 3)
    assert (pre[:, 0] != pre[:, 3]).any() and (pre[:, 1] != pre[:, 2]).any() and len(np.unique(outs[0][6])) >= 5 and len(np.unique(outs[0][7])) >= 5
    # and against the reference's own arrays read by the contract's rule: plane 0-2 = the sky at the direction
    want = er.cube_fetch(np.asarray(ref["sky"]), inp[:, 0:3], np.float32)
    helpers.assert_bits_equal_nan(np.ascontiguousarray(outs[0][0:3].T).view(np.uint32), np.ascontiguousarray(want).view(np.uint32), "CubeMap::fetch against env_reference.cube_fetch")
    E.close()


def test_composite_reads_sh9_from_device_memory(oracle, hr, ctx, env):
    """a 16 x 8 frame through hr_deferred_render with the env's device SH9 bound, with the same 36 floats in the params, and unbound again: one image"""
    import torch
    from hybrid_rendering_amd import api_deferred
    W, H = 16, 8
    P, levels, lut, n = 8, 4, 8, 64
    ref = _reference(env, "a", P, levels, lut, n)
    E = env.Environment(ctx, sky_size=8, prefiltered_size=P, prefiltered_levels=levels, brdf_lut_size=lut, n_samples=n)
    E.update(_f16(ref["sky"]))
    sd = helpers.scene_data("cornell")
    fr = helpers.make_frames(oracle, oracle.Scene(sd), "cornell", W, H, 1, 0.0)[0]
    sob, sr = synth.blue_noise_tables()
    fi = hr.frame_inputs(helpers.to_cuda(fr["gb"]), None, fr["ubo"], 0, 0, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda())
    g = api_deferred.DeferredShading(ctx, W, H)
    g.params.use_ray_traced_shadows = g.params.use_ray_traced_ao = g.params.use_ray_traced_reflections = g.params.use_ddgi = 0
    e = E.get()

    def render():
        g.render(fi, e)
        torch.cuda.synchronize()
        return helpers.bits16(g.output()).copy()

    without = render()                                   # params hold zeros, nothing bound: no ambient diffuse
    env.bind_sh9(g, E.sh9_device())
    bound = render()
    sh9 = E.read_sh9()
    assert np.array_equal(sh9.view(np.uint32), np.asarray(ref["sh9"]))
    env.bind_sh9(g, None)
    assert np.array_equal(render(), without)             # unbound again: the params' zeros
    g.set_sh9(sh9)
    through_params = render()
    env.bind_sh9(g, E.sh9_device())
    g.set_sh9(np.zeros((9, 4), np.float32))              # bound: the params' coefficients are not read
    bound_again = render()
    env.bind_sh9(g, None)
    g.set_sh9(sh9)
    unbound = render()
    assert np.array_equal(bound, through_params) and np.array_equal(bound_again, through_params) and np.array_equal(unbound, through_params)
    geometry = fr["gb"]["depth"] != 1.0
    assert geometry.any() and (bound[geometry] != without[geometry]).any()      # the coefficients do reach the image
    g.close()
    E.close()
