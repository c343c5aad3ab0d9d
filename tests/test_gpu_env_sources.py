"""hr_env_update_equirect and hr_env_update_sky on the device (csrc/env_sources.hip) against the numpy restatement of include/hr_env_sources.h
(tests/env_sources_reference.py): the equirect path bit for bit, fed the library's own table (tests/test_env_sources_host.py holds that table to
numpy's); the analytic sky within the header's tolerance of the float64 restatement; behind both, SH9 and the prefiltered chain bit for bit against
tests/env_reference.py over the sky the device holds — the same derived launches as hr_env_update.  Then the object's state across the three kinds
of update, graph capture, and what the reflections' miss and the composite's skybox read."""
import os

import numpy as np
import pytest

import env_reference as er
import env_sources_reference as esr
import helpers
from hybrid_rendering_amd import synth, synth_env

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LUT, N = 4, 64
_IMAGES, _REF = {}, {}


@pytest.fixture(scope="module")
def env(hr):
    from hybrid_rendering_amd import env as envmod
    return envmod


@pytest.fixture(scope="module")
def src(hr):
    from hybrid_rendering_amd import env_sources
    return env_sources


def _shape(S):
    """(prefiltered_size, levels): the whole chain down to 1 x 1; above 8 level 0 is a fetch, not a copy"""
    P = min(S, 8)
    return P, P.bit_length()


def _image(name):
    if not _IMAGES:
        _IMAGES.update(esr.equirect_images())
        from hybrid_rendering_amd import assets
        fix = assets.load_hdr(os.path.join(GOLDEN, "env_small.hdr")).copy()
        for k, val in enumerate((1e6, np.inf, np.nan, -1.0)):      # what a Radiance file cannot hold
            fix[(k * 7 + 3) % 32, (k * 37 + 63) % 64, k % 3] = val
        _IMAGES["64x32"] = fix
        for v in _IMAGES.values():
            v.setflags(write=False)
    return _IMAGES[name]


IMAGE_NAMES = ["1x1", "2x1", "8x4", "7x5", "64x32"]


def _derived(env, sky_u16, S):
    P, levels = _shape(S)
    return dict(sky=sky_u16, chain=er.prefiltered_chain(sky_u16, P, levels, env.sample_table(N)), sh9=er.sh9(sky_u16).view(np.uint32))


def _equirect_reference(env, src, S, name):
    """computed once per (size, image) and never modified"""
    if (S, name) not in _REF:
        r = _derived(env, esr.equirect_to_cube(src.equirect_table(S), _image(name)), S)
        for v in r.values():
            v.setflags(write=False)
        _REF[(S, name)] = r
    return _REF[(S, name)]


def _make(env, ctx, S):
    P, levels = _shape(S)
    return env.Environment(ctx, sky_size=S, prefiltered_size=P, prefiltered_levels=levels, brdf_lut_size=LUT, n_samples=N)


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # np.array: a writable copy (the shared images are read-only)


def _read(E):
    import torch
    torch.cuda.synchronize()
    return dict(sky=helpers.bits16(E.sky()), chain=helpers.bits16(E.prefiltered()), sh9=E.read_sh9().view(np.uint32))


def _assert_equal(got, ref, what):
    for k in ("sky", "chain", "sh9"):
        helpers.assert_bits_equal_nan(got[k], np.asarray(ref[k]), f"{what}: {k}")


def _pointers(E):
    e = E.get()
    return (e.sky, e.sky_size, e.prefiltered, e.prefiltered_size, e.prefiltered_levels, e.brdf_lut, e.brdf_lut_size, E.sh9_device())


@pytest.mark.parametrize("S", [4, 8, 16])
def test_equirect_cases_reach_the_wrap_and_both_pole_clamps(src, S):
    """from the library's table, with the kernel's own float32 addressing: some texel's left column is the map's last (x0 == w - 1, or x0 == -1), some
    texel's upper row is clamped at the north pole and some texel's lower row at the south pole — by a map with more than one column and row"""
    table = src.equirect_table(S)
    reached = {}
    for name in IMAGE_NAMES:
        h, w = _image(name).shape[:2]
        _, _, _, _, _, _, x0, y0 = esr.equirect_taps(table, w, h)
        assert x0.min() >= -1 and x0.max() <= w - 1 and y0.min() >= -1 and y0.max() <= h - 1
        reached[name] = (bool(((x0 == w - 1) | (x0 == -1)).any()), bool((y0 == -1).any()), bool((y0 + 1 == h).any()))
    assert reached["8x4"] == (True, True, True), reached
    assert all(reached["1x1"]) and all(any(r[k] for r in reached.values()) for k in range(3))


@pytest.mark.parametrize("name", IMAGE_NAMES)
@pytest.mark.parametrize("S", [4, 8, 16])
def test_equirect_matches_the_contract_bit_for_bit(hr, ctx, env, src, S, name):
    ref = _equirect_reference(env, src, S, name)
    E = _make(env, ctx, S)
    ptrs = _pointers(E)
    E.update_equirect(_cuda(_image(name)))
    got = _read(E)
    _assert_equal(got, ref, f"sky {S}, map {name}")
    assert _pointers(E) == ptrs
    val = got["sky"].view(np.float16).astype(np.float32)
    assert np.isfinite(val).all() and (val >= 0).all() and (val[..., 3] == 1.0).all()
    if S == 16 and name in ("8x4", "7x5"):
        assert (val[..., :3] == 65504.0).any()      # many cube texels per map texel: 1e6 and +inf are sampled, and saturate
    E.close()


def _sky_error(got_u16, ref):
    """max over texels and channels of |gpu - ref| / bound, bound = max(2^-10 * max(ref rgb), 2^-24)"""
    got = got_u16.view(np.float16)[..., :3].astype(np.float64)
    bound = np.maximum(2.0 ** -10 * ref.max(-1, keepdims=True), 2.0 ** -24)
    return float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("i", range(len(esr.SKY_SETS)))
@pytest.mark.parametrize("S", [4, 16, 32])
def test_sky_is_within_the_tolerance_of_the_float64_restatement(hr, ctx, env, S, i):
    """per texel and channel |gpu - ref| <= 2^-10 * max(ref_r, ref_g, ref_b), floor 2^-24 (include/hr_env_sources.h: the fp32 evaluation errs by a few
    1e-7 per term, the colour matrix cancels among terms of the size of the largest channel, the fp16 store adds at most half an ulp of the channel).
    Measured on MI355X, max error / bound over the 19 parameter sets and three sizes: see docs/EXPERIMENTS.md "Environment pipeline"."""
    params = esr.SKY_SETS[i]
    ref = esr.sky_reference(S, **params)
    E = _make(env, ctx, S)
    ptrs = _pointers(E)
    E.update_sky(**params)
    got = _read(E)
    worst = _sky_error(got["sky"], ref)
    print(f"sky S={S} set={i} {params}: max error / bound = {worst:.4f}")
    assert worst <= 1.0, (S, params, worst)
    assert (got["sky"][..., 3] == np.float16(1.0).view(np.uint16)).all() and _pointers(E) == ptrs
    if params.get("scale", 1.0) == 0.0:
        assert not got["sky"][..., :3].any()
    # the same derived launches as hr_env_update: SH9 and the chain of the sky the device holds
    _assert_equal(got, _derived(env, got["sky"], S), f"sky {S}, set {i}")
    E.close()


def test_state_across_the_three_kinds_of_update(hr, ctx, env, src):
    """update, update_equirect and update_sky interleaved on one env: each leaves exactly what it alone leaves on a fresh env"""
    S = 8
    cube = _cuda(synth_env.sky_cubemap(size=S)).view(__import__("torch").float16)
    img = _cuda(_image("7x5"))
    sky_params = esr.SKY_SETS[6]
    calls = dict(update=lambda E: E.update(cube), equirect=lambda E: E.update_equirect(img), sky=lambda E: E.update_sky(**sky_params))
    alone = {}
    for k, call in calls.items():
        F = _make(env, ctx, S)
        call(F)
        alone[k] = _read(F)
        F.close()
    _assert_equal(alone["equirect"], _equirect_reference(env, src, S, "7x5"), "a fresh env")
    assert not np.array_equal(alone["update"]["sky"], alone["sky"]["sky"]) and not np.array_equal(alone["equirect"]["sh9"], alone["sky"]["sh9"])
    E = _make(env, ctx, S)
    ptrs = _pointers(E)
    for k in ("sky", "equirect", "update", "equirect", "sky", "sky", "update", "sky", "equirect"):
        calls[k](E)
        _assert_equal(_read(E), alone[k], f"after {k}")
        assert _pointers(E) == ptrs
    E.close()


def test_capture_of_the_two_updates(hr, ctx, env, src):
    """the first equirect call on an env allocates and uploads its table: under capture it is refused and nothing of it reaches the graph; after an
    eager first call, {update_sky; update_equirect} is a graph whose replays read the map buffer's contents THEN.  update_sky's parameters are read
    when the call is made: every replay writes the sky of the capture"""
    import torch
    S = 8
    names = ["8x4", "8x4_b", "8x4_c"]
    rng = np.random.RandomState(5)
    maps = {"8x4": np.array(_image("8x4"))}
    for k in names[1:]:
        maps[k] = np.ones((4, 8, 4), np.float32)
        maps[k][..., :3] = rng.uniform(0.0, 4.0, (4, 8, 3)).astype(np.float32)
    table = src.equirect_table(S)
    refs = {k: _derived(env, esr.equirect_to_cube(table, maps[k]), S) for k in names}
    sky_params = esr.SKY_SETS[5]

    E = _make(env, ctx, S)
    buf, scratch = _cuda(maps["8x4"]), torch.zeros(4, device="cuda")
    stream, refused = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(refused, stream=stream):
        with pytest.raises(hr.HRError, match="capturing"):
            E.update_equirect(buf)
        scratch.add_(1.0)
    refused.replay()
    got = _read(E)
    assert scratch.tolist() == [1.0] * 4 and not got["sky"].any() and not got["chain"].any() and not got["sh9"].any()

    F = _make(env, ctx, S)
    F.update_sky(**sky_params)
    eager_sky = _read(F)
    F.close()

    E.update_equirect(buf)                                  # eager: builds the table
    _assert_equal(_read(E), refs["8x4"], "eager")
    views = dict(sky=E.sky(), chain=E.prefiltered(), sh9=E.sh9())
    kept = {k: torch.zeros_like(v) for k, v in views.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        E.update_sky(**sky_params)
        for k in views:
            kept[k].copy_(views[k])                         # what update_sky left, before update_equirect overwrites it
        E.update_equirect(buf)
    for k in ("8x4_b", "8x4_c", "8x4"):
        buf.copy_(_cuda(maps[k]))
        for v in kept.values():
            v.zero_()
        torch.cuda.synchronize()
        graph.replay()
        _assert_equal(_read(E), refs[k], f"replay with map {k}")
        mid = dict(sky=helpers.bits16(kept["sky"]), chain=helpers.bits16(kept["chain"]), sh9=kept["sh9"].cpu().numpy().view(np.uint32))
        _assert_equal(mid, eager_sky, f"replay with map {k}: the sky of the capture")
    E.close()


def test_consumers_read_the_equirect_sky(oracle, hr, ctx, env):
    """a Cornell frame: the reflections' trace (rays that leave through the open front read the sky or the chain) and the composite with its skybox
    stage, over an env fed by update_equirect and over an env fed the identical cubemap through hr_env_update — one image each; over an env that was
    never updated both differ, so the passes do read it"""
    import torch
    from hybrid_rendering_amd import api_deferred, api_gi, api_reflections
    W, H, S = 48, 32, 16
    sd = helpers.scene_data("cornell")
    gsc = hr.Scene(ctx, sd)
    fr = helpers.make_frames(oracle, oracle.Scene(sd), "cornell", W, H, 1, 0.0)[0]
    sky_px = fr["gb"]["depth"] == 1.0
    assert 0.05 < sky_px.mean() < 0.9
    envs = [_make(env, ctx, S) for _ in range(3)]
    envs[0].update_equirect(_cuda(_image("64x32")))
    torch.cuda.synchronize()
    cube = envs[0].sky().clone()
    envs[1].update(cube)
    _assert_equal(_read(envs[1]), _read(envs[0]), "hr_env_update with the cubemap update_equirect made")
    lo, hi = sd.bounds()
    ddgi = synth_env.ddgi_uniforms(lo, hi, probe_counts=(3, 3, 3), rays_per_probe=64, normal_bias=1.0)
    sob, sr = synth.blue_noise_tables()
    full_d = helpers.to_cuda(fr["gb"])
    fi = hr.frame_inputs(full_d, full_d, fr["ubo"], 0, 0, torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda(), cur_full=full_d)
    orient = synth_env.random_orientation(np.random.RandomState(7))
    outs = []
    for E in envs:
        e = E.get()
        g_gi, g_rf, g_df = api_gi.DDGI(ctx, W, H, ddgi), api_reflections.RayTracedReflections(ctx, W, H, 0), api_deferred.DeferredShading(ctx, W, H)
        g_gi.render(gsc, fi, e, orient)
        g_rf.render(gsc, fi, e, g_gi)
        env.bind_sh9(g_df, E.sh9_device())
        g_df.params.use_ray_traced_shadows = g_df.params.use_ray_traced_ao = g_df.params.use_ddgi = 0
        g_df.params.use_ray_traced_reflections = 1
        g_df.render(fi, e, reflections=g_rf.output(hr.OUTPUT_UPSAMPLE))
        torch.cuda.synchronize()
        outs.append((helpers.bits16(g_rf.image(g_rf.IMG_TRACE)).copy(), helpers.bits16(g_df.output()).copy()))
        g_df.close(); g_rf.close(); g_gi.close()
    for k, what in ((0, "reflections trace"), (1, "composite")):
        helpers.assert_bits_equal_nan(outs[0][k], outs[1][k], what)
        assert (outs[0][k] != outs[2][k]).any(), what
    comp = outs[0][1]
    assert (comp[sky_px] != outs[2][1][sky_px]).any() and oracle.f16(comp[sky_px][:, :3]).max() > 0      # the skybox stage shows the map
    for E in envs:
        E.close()
    gsc.close()
