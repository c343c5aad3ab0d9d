"""The device shading layer against the oracle, function by function: hr_selftest_shading (csrc/selftest_shading.hip — shading.h, cutout.h and
sampling.h through the product's own functions) and its mirror orc_selftest_shading on the families of tests/shading_cases.py, bit for bit with
NaN == NaN.  tests/test_shading_cases.py (CPU) shows that the families reach what they are named for and that the oracle agrees with a float64
restatement; the two forks of the sampling code (k_deferred's inline level selection and LUT lookup, the AO trace's own cosine lobe) run through
their passes at the bottom."""
import ctypes as C

import numpy as np
import pytest

import helpers
import shading_cases as sc

pytestmark = pytest.mark.gpu


def _device(hr, mode, case, dev_tables):
    import torch
    from oracle import pyoracle as po
    key = (case.tables.get("key"), id(case.tables))
    if key not in dev_tables:      # one upload per table set
        keep = {n: torch.from_numpy(np.ascontiguousarray(case.tables[n]).view(np.uint8).reshape(-1).copy()).cuda() for n in po.SHADING_POINTERS if case.tables.get(n) is not None}
        dev_tables[key] = (keep, po.shading_tables(case.tables, address={n: t.data_ptr() for n, t in keep.items()}))
    keep, tab = dev_tables[key]
    x = torch.from_numpy(case.inp).cuda()
    out = torch.full((case.nout, len(case.inp)), 7.0, dtype=torch.float32, device="cuda")
    st = hr.lib().hr_selftest_shading(C.c_int32(mode), C.c_int64(len(case.inp)), C.c_void_p(x.data_ptr()), C.c_void_p(C.addressof(tab)), C.c_int32(case.nout),
                                      C.c_void_p(out.data_ptr()), None)
    assert st == 0, (case.name, hr.lib().hr_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_mode(hr, oracle, mode):
    dev_tables = {}
    problems = []
    for case in sc.cases(mode):
        got = _device(hr, mode, case, dev_tables)
        ref = oracle.selftest_shading(mode, case.inp, case.tables, case.nout)
        g, r = got.view(np.uint32), ref.view(np.uint32)
        bad = ((g != r) & ~(np.isnan(got) & np.isnan(ref))).any(0)
        if bad.any():
            i = np.flatnonzero(bad)[:4]
            problems.append(f"{case.name}: {int(bad.sum())} of {len(case.inp)} elements differ; first {i.tolist()} in {case.inp[i].tolist()} "
                            f"device {got[:, i].T.tolist()} oracle {ref[:, i].T.tolist()}")
        for plane, want in case.expect.items():      # a tie family's written-down outcome, on the device itself
            helpers.assert_bits_equal_nan(got[plane].view(np.uint32), want.view(np.uint32), f"{case.name} plane {plane} against the documented priority")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("mode", range(12), ids=sc.MODE_NAMES)
def test_shading_layer_matches_the_oracle_bit_for_bit(hr, oracle, mode):
    _check_mode(hr, oracle, mode)


def test_selftest_shading_rejects_what_its_clamps_assume(hr):
    """a table block whose extents the kernels' clamps could not hold is an error before any launch"""
    from oracle import pyoracle as po
    case = sc.cases(sc.CUBE)[0]
    arrays = {k: v for k, v in case.tables.items() if k not in po.SHADING_POINTERS}
    tab = po.shading_tables(arrays)      # no tables at all
    for mode in (sc.CUBE, sc.TEXTURE, sc.GATHER, sc.SURFACE):
        assert hr.lib().hr_selftest_shading(C.c_int32(mode), C.c_int64(0), None, C.c_void_p(C.addressof(tab)), C.c_int32(1), None, None) == 1, mode
    assert hr.lib().hr_selftest_shading(C.c_int32(99), C.c_int64(0), None, C.c_void_p(C.addressof(tab)), C.c_int32(1), None, None) == 1


# ---- the two forks of the sampling code, through their passes ------------------------------------------------------------------------------
def _f16bits(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def test_deferred_inline_level_selection_and_lut_lookup_match_the_oracle(oracle, hr, ctx):
    """k_deferred restates EnvDev's level selection and LUT lookup inline.  A synthetic 32 x 8 G-buffer: the roughness column enumerates the level
    ties roughness * 4 + 0.5 (on the integer and the fp16 neighbours either side), 0, 1 and values past both ends of the chain; the rows enumerate
    normals toward, across and away from the viewer (NdotV from ~1 down to the 0 clamp).  A 4 x 3-level chain whose texels name their level, and a
    size-1 LUT: every index must land on its one texel."""
    import torch
    from hybrid_rendering_amd import api_deferred, api_gi, synth
    from oracle import pyoracle_deferred as odf
    W, H = 32, 8
    ties = np.array([0.125, 0.375, 0.625, 0.875], np.float16)
    rough = np.array([int(t.view(np.uint16)) + k for t in ties for k in (-1, 0, 1)], np.uint16).view(np.float16)
    rough = np.concatenate([rough, np.array([0.0, -0.0, 1.0, 0.999, 1.5, 4.0, 100.0, -0.25, 0.05, 0.1, 0.2, 0.3, 0.45, 0.5, 0.55, 0.7, 0.75, 0.8, 0.9, 0.95], np.float16)])
    assert len(rough) == W
    level = np.clip(np.floor((rough.astype(np.float32) * np.float32(4) + np.float32(0.5)).astype(np.float32)), 0, 2)
    assert all((level == k).any() for k in range(3)) and (rough.astype(np.float32) * 4 + 0.5 == np.array([1, 2, 3, 4], np.float32)[:, None]).any(1).all()
    normals = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0.6, 0, 0.8], [0.0, 0.8, -0.6]], np.float32)
    oct_ = oracle.selftest_math(0, 6, H, np.concatenate([normals, np.zeros((H, 5), np.float32)], 1), nout=2).T      # direction_to_octohedral
    gb = dict(gb1=np.zeros((H, W, 4), np.uint8), gb2=np.zeros((H, W, 4), np.uint16), gb3=np.zeros((H, W, 4), np.uint16), depth=np.zeros((H, W), np.float32))
    rng = np.random.RandomState(5)
    gb["gb1"][..., 0:3] = rng.randint(40, 255, (H, W, 3))
    gb["gb1"][..., 3] = rng.choice([0, 128, 255], (H, W))
    gb["gb2"][..., 0:2] = _f16bits(oct_)[:, None, :]
    gb["gb3"][..., 0] = rough.view(np.uint16)[None, :]
    gb["depth"][:] = rng.uniform(0.9, 0.999, (H, W))
    cam = synth.cornell_camera(W / H)
    ubo = synth.make_ubo(cam, None, synth.cornell_light(hard=True))
    T = sc.cube_tables(1, 4, 3, 1)
    pre = T["prefiltered"].reshape(-1, 4).copy()
    lut = _f16bits(np.array([[[0.5, 0.25]]]))
    sky = np.ascontiguousarray(T["cube"])
    env_np = dict(sky=sky, prefiltered=pre, pre_size=4, pre_levels=3, lut=lut)
    f16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().view(torch.float16)
    env = api_gi.environment(f16(sky), f16(pre), 4, 3, f16(lut))
    sob, sr = synth.blue_noise_tables()
    fi = hr.frame_inputs(helpers.to_cuda(gb), None, ubo, 0, 0, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda())
    g = api_deferred.DeferredShading(ctx, W, H)
    g.params.use_ray_traced_shadows = g.params.use_ray_traced_ao = g.params.use_ray_traced_reflections = g.params.use_ddgi = 0
    g.params.draw_skybox = 0
    g.render(fi, env)
    torch.cuda.synchronize()
    got = helpers.bits16(g.output()).copy()
    ref = odf.shade(ubo, gb, None, None, None, None, 0, np.zeros((9, 4), np.float32), env_np, skybox=False)
    helpers.assert_bits_equal_nan(got, ref, "deferred composite on the level ties and LUT edges")
    # the chain's texels name their level: the specular term's red channel is (8 * level + face) * (F * 0.5 + 0.25) * 2, so two roughness columns of
    # different levels differ somewhere — the fetch really moved between levels across each tie
    val = got.view(np.float16).astype(np.float32)
    for t in ties:
        below, on = (rough.view(np.uint16) == int(t.view(np.uint16)) - 1), (rough == t)
        assert (val[:, below.argmax(), 0] != val[:, on.argmax(), 0]).any(), t
    # an environment whose chain ends before its last level has a texel is an error, not a fetch in front of the level
    bad = api_gi.environment(f16(sky), f16(pre), 4, 4, f16(lut))
    for e in (bad, api_gi.environment(f16(sky), f16(pre), 0, 3, f16(lut)), api_gi.environment(f16(sky), f16(pre), -4, 1, f16(lut))):
        st = hr.lib().hr_deferred_render(g.h, C.byref(fi), C.byref(e), None, None, None, None, C.byref(g.params), None)
        assert st == 1 and b"prefiltered" in hr.lib().hr_last_error(), (st, hr.lib().hr_last_error())      # HR_ERR_INVALID_ARG, before any launch
    g.close()


def test_reflections_reject_a_prefiltered_chain_without_a_last_texel(oracle, hr, ctx):
    import torch
    from hybrid_rendering_amd import api_gi, api_reflections, synth, synth_env
    sd = helpers.scene_data("cornell")
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
    W = H = 32
    fr = helpers.make_frames(oracle, osc, "cornell", W, H, 1, 0.0)[0]
    lo, hi = sd.bounds()
    g_ddgi = api_gi.DDGI(ctx, W, H, synth_env.ddgi_uniforms(lo, hi, probe_counts=(2, 2, 2), rays_per_probe=32, normal_bias=1.0))
    T = sc.cube_tables(1, 4, 3, 1)
    f16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().view(torch.float16)
    sky, pre, lut = f16(T["cube"]), f16(T["prefiltered"].reshape(-1, 4)), f16(T["lut"])
    sob, sr = synth.blue_noise_tables()
    cur = helpers.to_cuda(fr["gb"])
    fi = hr.frame_inputs(cur, cur, fr["ubo"], 0, 0, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda(), cur_full=cur)
    gp = api_reflections.RayTracedReflections(ctx, W, H, 0)
    gp.params.sample_gi = 1
    for size, levels in ((4, 4), (0, 3), (-4, 1), (4, 40)):
        e = api_gi.environment(sky, pre, size, levels, lut)
        st = hr.lib().hr_reflections_render(gp.h, gsc.h, C.byref(fi), C.byref(e), g_ddgi.h, C.byref(gp.params), None)
        assert st == 1 and b"prefiltered" in hr.lib().hr_last_error(), (size, levels, st, hr.lib().hr_last_error())
    gp.close()
    g_ddgi.close()
    gsc.close()


def test_ao_trace_lobe_on_its_basis_threshold_matches_the_oracle(oracle, hr, ctx):
    """ao.hip keeps its own sample_cosine_lobe (max2 where shading.h's has the specification's max).  The AO trace on a Cornell G-buffer whose normals
    are rewritten to the fp16 oct codes that decode closest to |N.y| = 0.99 from either side — as near the lobe's basis threshold as a G-buffer
    can put a normal — in both signs of y."""
    import torch
    from hybrid_rendering_amd import synth
    sd = helpers.scene_data("cornell")
    osc, gsc = oracle.Scene(sd), hr.Scene(ctx, sd)
    W = H = 64
    fr = helpers.make_frames(oracle, osc, "cornell", W, H, 1, 0.0)[0]
    # oct codes (ex, ey) with ex small: N ~ (ex, ey, 1 - |ex| - |ey|) normalised; ey runs over every fp16 value of a window around the crossing
    ey = np.arange(np.float16(0.84).view(np.uint16), np.float16(0.91).view(np.uint16), dtype=np.uint16).view(np.float16)
    ex = np.array([0.0, 0.01, -0.02], np.float16)
    code = np.array([(a, s * b) for s in (1, -1) for a in ex for b in ey], np.float16)
    dec = oracle.selftest_math(0, 5, len(code), np.concatenate([code.astype(np.float32), np.zeros((len(code), 6), np.float32)], 1), nout=3).T
    ny = np.abs(dec[:, 1])
    near = np.argsort(np.abs(ny - np.float32(0.99)))[: W * H // 4]
    assert (ny[near] > np.float32(0.99)).sum() > 100 and (ny[near] <= np.float32(0.99)).sum() > 100 and np.abs(ny[near] - 0.99).min() < 2e-4 and (dec[near, 1] < 0).any()
    gb = {k: v.copy() for k, v in fr["gb"].items()}
    geo = np.argwhere(gb["depth"] != 1.0)
    rng = np.random.RandomState(11)
    pick = near[rng.randint(0, len(near), len(geo))]
    gb["gb2"][geo[:, 0], geo[:, 1], 0] = code[pick, 0].view(np.uint16)
    gb["gb2"][geo[:, 0], geo[:, 1], 1] = code[pick, 1].view(np.uint16)
    sob, sr = synth.blue_noise_tables()
    gp = hr.RayTracedAO(ctx, W, H, 0)
    cur = helpers.to_cuda(gb)
    fi = hr.frame_inputs(cur, cur, fr["ubo"], 0, 0, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda(), z_buffer_params=synth.z_buffer_params())
    gp.ray_trace(gsc, fi)
    torch.cuda.synchronize()
    mh = (H + 3) // 4
    mask = gp.image(gp.IMG_MASK).cpu().numpy().view(np.uint32)[:mh].reshape(mh, -1)
    ref, rays = oracle.ao_ray_trace(osc, fr["ubo"], gb["depth"], gb["gb2"], sob, sr, bias=gp.params.bias, ray_length=gp.params.ray_length, num_frames=0)
    assert np.array_equal(mask, ref[0]), f"{int((mask != ref[0]).sum())} mask words differ"
    bits = helpers.unpack_mask(ref[0], W, H)
    assert 0.05 < bits.mean() < 0.95          # the rays do meet geometry: the basis matters
    gp.close()
    gsc.close()
