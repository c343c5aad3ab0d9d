"""The probe-grid visualisation on the GPU (include/hr_probe_vis.h, csrc/probe_vis.hip) against the numpy restatement of its contract
(tests/probe_vis_reference.py: brute force over all probes) — colour, depth_out and probe_id_out bit for bit on every case of
tests/probe_vis_cases.py, with depth_out aliased onto depth_in, across the two walks, through hr_deferred_render_probes, and captured."""
import ctypes as C

import numpy as np
import pytest

import helpers
import probe_vis_cases as pc
import probe_vis_reference as ref
from hybrid_rendering_amd import synth, synth_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pv(hr):
    from hybrid_rendering_amd import probe_vis
    return probe_vis


def _f16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.float16)


def _run(pv, ctx, name, alias=False, radius=None):
    """one case through hr_probe_vis_render -> (colour bits, depth_out, ids)"""
    import torch
    b = pc.build(name)
    c = b["case"]
    color, depth_in = _f16(b["color"]), torch.from_numpy(b["depth_in"]).cuda()
    depth_out = depth_in if alias else torch.full_like(depth_in, -7.0)
    ids = torch.full((c.h, c.w), -9, dtype=torch.int32, device="cuda")
    pv.render(ctx, b["ubo"], b["grid"], _f16(b["irradiance"]), depth_in, color, depth_atlas=_f16(b["depth_atlas"]) if c.what == 1 else None,
              radius=c.radius if radius is None else radius, what=c.what, depth_out=depth_out, probe_id_out=ids)
    torch.cuda.synchronize()
    if not alias:
        assert np.array_equal(depth_in.cpu().numpy().view(np.uint32), b["depth_in"].view(np.uint32)), "depth_in was written"
    return helpers.bits16(color), depth_out.cpu().numpy(), ids.cpu().numpy()


def _assert_equal(got, want, what):
    col, dep, ids = got
    assert np.array_equal(ids, want["probe_id"]), f"{what}: {(ids != want['probe_id']).sum()} probe ids differ"
    assert np.array_equal(dep.view(np.uint32), want["depth_out"].view(np.uint32)), f"{what}: {(dep.view(np.uint32) != want['depth_out'].view(np.uint32)).sum()} depths differ"
    nan_g, nan_w = np.isnan(col.view(np.float16)), np.isnan(want["color"].view(np.float16))
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN positions differ"
    assert np.array_equal(col[~nan_g], want["color"][~nan_w]), f"{what}: {(col[~nan_g] != want['color'][~nan_w]).sum()} colour halfs differ"


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_case_equals_the_contract(pv, ctx, name):
    want = pc.expected(name)
    _assert_equal(_run(pv, ctx, name), want, name)
    _assert_equal(_run(pv, ctx, name, alias=True), want, name + " (depth_out aliases depth_in)")


def test_outputs_are_optional(pv, ctx):
    import torch
    b = pc.build("outside_near_r1")
    color = _f16(b["color"])
    pv.render(ctx, b["ubo"], b["grid"], _f16(b["irradiance"]), torch.from_numpy(b["depth_in"]).cuda(), color, radius=1.0)
    torch.cuda.synchronize()
    assert np.array_equal(helpers.bits16(color), pc.expected("outside_near_r1")["color"])


@pytest.mark.parametrize("pair", pc.PATH_PAIRS)
def test_walk_and_brute_force_agree(pv, ctx, pair):
    """r = half a step takes the lattice walk, the next float above it tests every probe: wherever the contract names the same probe for both
    radii, so do the two paths"""
    a, b = pair
    ids_a, ids_b = _run(pv, ctx, a)[2], _run(pv, ctx, b)[2]
    same = pc.expected(a)["probe_id"] == pc.expected(b)["probe_id"]
    assert same.mean() > 0.99 and np.array_equal(ids_a[same], ids_b[same])
    assert np.array_equal(ids_a, pc.expected(a)["probe_id"]) and np.array_equal(ids_b, pc.expected(b)["probe_id"])


def test_deferred_render_probes_equals_the_stateless_call(hr, pv, ctx):
    """a small Cornell frame after two DDGI frames: hr_deferred_render + hr_deferred_render_probes equals hr_probe_vis_render composed by hand from
    hr_ddgi_current_read over a copy of the plain composite; texels no sphere covers are the plain composite's"""
    import torch
    from hybrid_rendering_amd import api_deferred, api_gi
    W, H = 64, 48
    sd = helpers.scene_data("cornell")
    scene = hr.Scene(ctx, sd)
    lo, hi = sd.bounds()
    grid = synth_env.ddgi_uniforms(lo, hi, probe_counts=(4, 4, 4), rays_per_probe=32)
    radius = 0.2 * float(grid["grid_step"].min())
    ubo = synth.make_ubo(synth.cornell_camera(aspect=W / H), None, synth.cornell_light())
    sky = synth_env.sky_cubemap(16)
    pre, lut, sh9 = synth_env.prefiltered_chain(sky, 5), synth_env.brdf_lut(16), synth_env.sh9_from_cubemap(sky)
    env = api_gi.environment(_f16(sky), _f16(pre), 16, 5, _f16(lut))
    sob, sr = synth.blue_noise_tables()
    g = scene.gbuffer(ubo, W, H)
    fi = hr.frame_inputs(g, None, ubo, 0, 0, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda())
    ddgi = api_gi.DDGI(ctx, W, H, grid)
    rng = np.random.RandomState(3)
    for _ in range(2):
        ddgi.render(scene, fi, env, synth_env.random_orientation(rng))
    df = api_deferred.DeferredShading(ctx, W, H)
    df.set_sh9(sh9)
    df.params.use_ray_traced_shadows = df.params.use_ray_traced_ao = df.params.use_ray_traced_reflections = 0
    df.render(fi, env, gi=ddgi.output())
    plain = df.output().clone()
    for what in (0, 1):
        df.render(fi, env, gi=ddgi.output())
        depth_out = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        ids = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        df.render_probes(fi, ddgi, radius=radius, what=what, depth_out=depth_out, probe_id_out=ids)
        irr, dep = ddgi.current_read()
        by_hand, d2, i2 = plain.clone(), torch.zeros_like(depth_out), torch.zeros_like(ids)
        pv.render(ctx, ubo, grid, irr, g["depth"], by_hand, depth_atlas=dep, radius=radius, what=what, depth_out=d2, probe_id_out=i2)
        torch.cuda.synchronize()
        got, idn = helpers.bits16(df.output()), ids.cpu().numpy()
        assert np.array_equal(got, helpers.bits16(by_hand)) and np.array_equal(idn, i2.cpu().numpy()) and torch.equal(depth_out, d2)
        assert 0.02 < (idn >= 0).mean() < 0.9 and len(np.unique(idn[idn >= 0])) >= 5
        assert np.array_equal(got[idn < 0], helpers.bits16(plain)[idn < 0]) and (got[idn >= 0] != helpers.bits16(plain)[idn >= 0]).any()
        # and the stateless call over these atlases is the contract
        want = ref.render(ubo, grid, helpers.bits16(irr), helpers.bits16(dep), radius, what, g["depth"].cpu().numpy(), helpers.bits16(plain))
        _assert_equal((got, depth_out.cpu().numpy(), idn), want, f"cornell what={what}")
    for p in (df, ddgi, scene):
        p.close()


def _hip():
    """the HIP runtime this process already has loaded (the library's and torch's): never a second copy"""
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    L = C.CDLL(paths.pop())
    for f in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphGetNodes", "hipGraphNodeGetType", "hipGraphInstantiate", "hipGraphLaunch", "hipGraphExecDestroy",
              "hipGraphDestroy", "hipGraphNodeGetDependencies"):
        getattr(L, f).restype = C.c_int
    return L


def test_one_capture_follows_the_atlas(pv, ctx):
    """the call captured once into a hipGraph: one kernel node and nothing else; two replays over a changed atlas (and a restored image) give what
    the contract gives for each atlas"""
    import torch
    name = "outside_near_r1"
    b = pc.build(name)
    color0 = _f16(b["color"])
    color, depth_in, irr = color0.clone(), torch.from_numpy(b["depth_in"]).cuda(), _f16(b["irradiance"])
    ids = torch.zeros((b["case"].h, b["case"].w), dtype=torch.int32, device="cuda")
    depth_out = torch.zeros_like(depth_in)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    hip, sp = _hip(), C.c_void_p(stream.cuda_stream)
    graph, gexec, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    assert hip.hipStreamBeginCapture(sp, C.c_int(2)) == 0                      # hipStreamCaptureModeRelaxed
    try:
        pv.render(ctx, b["ubo"], b["grid"], irr, depth_in, color, radius=1.0, depth_out=depth_out, probe_id_out=ids, stream=stream)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1
    node, kind, ndep = (C.c_void_p * 1)(), C.c_int(-1), C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph, node, C.byref(n)) == 0 and hip.hipGraphNodeGetType(C.c_void_p(node[0]), C.byref(kind)) == 0 and kind.value == 0   # a kernel
    assert hip.hipGraphNodeGetDependencies(C.c_void_p(node[0]), None, C.byref(ndep)) == 0 and ndep.value == 0
    assert (ids == 0).all() and torch.equal(color, color0)                      # captured, not run
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    rng = np.random.RandomState(9)
    for k in range(2):
        atlas = b["irradiance"] if k == 0 else rng.uniform(0.0, 9.0, b["irradiance"].shape).astype(np.float16).view(np.uint16)
        irr.copy_(_f16(atlas))
        color.copy_(color0)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(gexec, sp) == 0
        stream.synchronize()
        want = ref.render(b["ubo"], b["grid"], atlas, b["depth_atlas"], 1.0, 0, b["depth_in"], b["color"])
        _assert_equal((helpers.bits16(color), depth_out.cpu().numpy(), ids.cpu().numpy()), want, f"replay {k}")
        if k:
            assert (want["color"] != pc.expected(name)["color"]).mean() > 0.2
    assert hip.hipGraphExecDestroy(gexec) == 0 and hip.hipGraphDestroy(graph) == 0
