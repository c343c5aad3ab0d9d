"""The bits of the tolerance-mode (exact = 0) denoise chains, pinned: SHA-256 digests of every stage image in tests/golden/fast_filters.json.

tests/test_gpu_golden.py pins the parity mode only; this module pins what bench.py times.  The digests were recorded from the library
as it stood BEFORE the filters of csrc/denoise_fast_*.hip (then one file) were moved into shared bodies (csrc/atrous_filters.h), so the module is the proof
that the move changed no bit.  Tolerance-mode arithmetic is ALLOWED to change later: a pull request that changes it on purpose re-records the
fixture (`python tests/test_gpu_fast_filters.py --record`, on the GPU) and says so in its description.  HR_LIBRARY selects the library.

Shape: the pass image is 138 x 76 (both ragged: no multiple of 32 or 8; five workgroup columns, ten tile rows — at tap distance 8 the
workgroups of columns 1-3 / rows 1-7 take the interior path, the others the edge path), three frames with a moving camera, inputs made as
in tests/test_gpu_fused.py.  `band` cases hold rows 16..56 with a halo of 8 (y0 = 8 > 0: the resident-row rules bite); only resident rows
are hashed.  A digest covers one stage image of all three frames.  Cases marked `stages` run, after render(), every a-trous iteration
again through the stage entry point (the unfused launches, same inputs) and pin each iteration's image; AO `stages` cases run the whole
pass through its stage entry points.

Kernel instantiations of the product library's launch_*_fast, and the case that reaches each:
  kf_shadows_temporal<0 | 1>            every shadows case: frame 0 | frames 1, 2 (the records stand in for the previous G-buffer)
  kf_shadows_atrous01<16, true>         shadows/fused, band, radius-1 cases with phi_normal 32
  kf_shadows_atrous01<16, false>        shadows/fused_phi12_iter5
  kf_shadows_atrous_lds<1 | 2, true>    shadows/unfused, unfused_band (and the `stages` re-run of every case)
  kf_shadows_atrous_lds<1 | 2, false>   shadows/unfused_phi12
  kf_shadows_atrous<4 | 8, true>        shadows/fused, unfused, band, iter5, half
  kf_shadows_atrous<4 | 8, false>       shadows/fused_phi12_iter5, unfused_phi12
  kf_shadows_atrous<0, true>            shadows/iter5 (tap distance 16, radius 1), radius2 (every iteration)
  kf_shadows_atrous<0, false>           shadows/fused_phi12_iter5 (tap distance 16), radius2_phi12
  kf_ao_temporal<false, 0 | 2>          ao/fused, unfused: frame 0 | frames 1, 2
  kf_ao_temporal<true, 0 | 2>           ao/radius6_spp2, half_radius2_spp2
  kf_ao_temporal<false | true, 1>       ao/band | ao/unfused_band_spp2 (frames 1, 2)
  kf_ao_blur_xy<4, 16>                  ao/fused, band
  kf_ao_blur<4>                         ao/unfused, unfused_band_spp2 (X and Y)
  kf_ao_blur_generic                    ao/radius6_spp2, half_radius2_spp2
  kf_refl_temporal<0 | 1>               every reflections case: frame 0 | frames 1, 2 (0 in every frame of unfused_norecords)
  kf_refl_atrous01<16, true | false>    reflections/fused, band, half | fused_phi8
  kf_refl_atrous<1 | 2, true | false>   reflections/unfused, unfused_norecords | unfused_phi8
  kf_refl_atrous<4 | 8, true | false>   reflections/fused, unfused, ... | fused_phi8, unfused_phi8
  kf_refl_atrous<0, true | false>       reflections/radius2 | radius2_phi8
  a.geo set | null                      reflections/unfused (records) | unfused_norecords (HR_GEO_HISTORY=0), and always null in atrous_01
  kf_ddgi_sample                        every reflections case (the DDGI pass runs in tolerance mode; its output is pinned)
  kf_upsample<1> | <4>                  shadows/half, ao/half_radius2_spp2 | reflections/half
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "fast_filters.json")
W, H, FRAMES = 138, 76, 3
BAND = (16, 56, 8, 8)   # band rows, halo, history halo: resident rows 8..64

# name -> (creation switches, parameters)
SHADOWS = {
    "fused":             (dict(), dict()),
    "unfused":           (dict(fuse=0, stages=True), dict()),
    "fused_phi12_iter5": (dict(), dict(phi_normal=12.5, filter_iterations=5, power=2.0, feedback_iteration=0)),
    "unfused_phi12":     (dict(fuse=0, stages=True), dict(phi_normal=12.5, power=0.0, feedback_iteration=0)),
    "iter5":             (dict(stages=True), dict(filter_iterations=5, power=0.0)),
    "radius2":           (dict(stages=True), dict(radius=2, power=2.0)),
    "radius2_phi12":     (dict(), dict(radius=2, phi_normal=12.5, feedback_iteration=0)),
    "band":              (dict(band=True), dict()),
    "unfused_band":      (dict(band=True, fuse=0, stages=True), dict(power=2.0)),
    "half":              (dict(scale=1), dict()),
    "cornell":           (dict(scene="cornell", stages=True), dict(power=0.0, feedback_iteration=0)),
}
AO = {
    "fused":              (dict(), dict(blur_radius=4)),
    "unfused":            (dict(stages=True), dict(blur_radius=4)),
    "radius6_spp2":       (dict(), dict(blur_radius=6, spp=2)),
    "band":               (dict(band=True), dict(blur_radius=4)),
    "unfused_band_spp2":  (dict(band=True, stages=True), dict(blur_radius=4, spp=2)),
    "half_radius2_spp2":  (dict(scale=1), dict(blur_radius=2, spp=2)),
    "cornell":            (dict(scene="cornell"), dict(blur_radius=4)),
}
REFLECTIONS = {
    "fused":             (dict(), dict()),
    "fused_phi8":        (dict(stages=True), dict(phi_normal=8.0, blur_as_input=1, feedback_iteration=0)),
    "unfused":           (dict(fuse=0, stages=True), dict(blur_as_input=1, feedback_iteration=1)),
    "unfused_phi8":      (dict(fuse=0), dict(phi_normal=8.0, approximate_with_ddgi=0)),
    "unfused_norecords": (dict(fuse=0, records=0), dict()),
    "radius2":           (dict(stages=True), dict(radius=2)),
    "radius2_phi8":      (dict(), dict(radius=2, phi_normal=8.0, blur_as_input=1)),
    "band":              (dict(band=True), dict()),
    "half":              (dict(scale=1), dict()),
}


def _modules():
    import helpers
    from hybrid_rendering_amd import api, api_gi, api_reflections, synth, synth_env
    return helpers, api, api_gi, api_reflections, synth, synth_env


_worlds = {}


def _world(ctx, name, scale, mirror):
    """scene + three frames of inputs, made once per (scene, scale) and shared by the cases; `mirror`: the reflections' own copy, with the
    polished materials' roughness lowered so that the mirror regime exists (tests/test_gpu_fused.py)"""
    key = (name, scale, mirror)
    if key not in _worlds:
        import torch
        helpers, hr, _, _, synth, _ = _modules()
        gsc = hr.Scene(ctx, helpers.scene_data(name))
        FW, FH = W << scale, H << scale
        cams = helpers.cameras(name, FW / FH, FRAMES + 1, 1.5)
        light = helpers.light_for(name)
        ubos = [synth.make_ubo(cams[i + 1], cams[i], light) for i in range(FRAMES)]
        gbs = [gsc.gbuffer(u, FW, FH) for u in ubos]
        if mirror:
            for g in gbs:
                ch = g["gb3"][..., 0]
                ch[ch == 0.1] = 0.03
        lows = [hr.gbuffer_mip(g, scale) for g in gbs] if scale else gbs
        sob, sr = synth.blue_noise_tables()
        _worlds[key] = dict(gsc=gsc, ubos=ubos, gbs=gbs, lows=lows, sob=torch.from_numpy(sob).cuda(), sr=torch.from_numpy(sr).cuda())
    return _worlds[key]


class _Digests:
    """stage name -> SHA-256 over the stage image's raw bytes, frame after frame; `rows`: the resident rows of a band"""

    def __init__(self, rows):
        self.h, self.rows = {}, rows

    def add(self, stage, t, tiles=False, full=False):
        a = t.contiguous().cpu().numpy()
        if self.rows and not full:
            y0, y1 = self.rows
            a = a[y0 // 8:(y1 + 7) // 8] if tiles else a[y0:y1]
        self.h.setdefault(stage, hashlib.sha256()).update(np.ascontiguousarray(a).tobytes())

    def result(self):
        return {k: v.hexdigest() for k, v in sorted(self.h.items())}


def _create(make, sw):
    """the pass, created under the developer switches its hr_*_create reads once: HR_FUSE, HR_GEO_HISTORY"""
    env = {}
    if "fuse" in sw:
        env["HR_FUSE"] = str(sw["fuse"])
    if "records" in sw:
        env["HR_GEO_HISTORY"] = str(sw["records"])
    os.environ.update(env)
    try:
        return make()
    finally:
        for k in env:
            del os.environ[k]


def _setup(ctx, sw, mirror=False):
    scale = sw.get("scale", 0)
    wd = _world(ctx, sw.get("scene", "sponza_small"), scale, mirror)
    band = BAND if sw.get("band") else None
    rows = (max(0, BAND[0] - BAND[2]), min(H, BAND[1] + BAND[2])) if band else None
    return wd, scale, band, _Digests(rows)


def _inputs(hr, wd, f, scale, **kw):
    if scale:
        kw["cur_full"] = wd["gbs"][f]
    return hr.frame_inputs(wd["lows"][f], wd["lows"][f - 1 if f else 0], wd["ubos"][f], f, f & 1, wd["sob"], wd["sr"], **kw)


def run_shadows(ctx, case):
    import torch
    _, hr, *_ = _modules()
    sw, params = SHADOWS[case]
    wd, scale, band, dg = _setup(ctx, sw)
    p = _create(lambda: hr.RayTracedShadows(ctx, W << scale, H << scale, scale, band=band), sw)
    p.params.exact = 0
    for k, v in params.items():
        setattr(p.params, k, v)
    for f in range(FRAMES):
        fi = _inputs(hr, wd, f, scale)
        p.render(wd["gsc"], fi)
        torch.cuda.synchronize()
        dg.add("temporal", p.image(p.IMG_TEMPORAL))
        dg.add("tiles", p.image(p.IMG_TILES), tiles=True)
        dg.add("atrous0", p.image(p.IMG_ATROUS0))
        dg.add("atrous1", p.image(p.IMG_ATROUS1))
        dg.add("feedback", p.image(p.IMG_PREV))
        dg.add("output", p.output(hr.OUTPUT_ATROUS))
        if scale:
            dg.add("upsample", p.output(hr.OUTPUT_UPSAMPLE), full=True)
        if sw.get("stages"):
            for i in range(p.params.filter_iterations):
                p.atrous_iteration(fi, i)
                torch.cuda.synchronize()
                dg.add(f"iteration{i}", p.image(p.IMG_ATROUS0 if i & 1 else p.IMG_ATROUS1))
    v = p.output(hr.OUTPUT_ATROUS)[slice(*dg.rows) if dg.rows else slice(None)][..., 0].float().cpu().numpy()
    assert 0.02 < (v > 0).mean() < 0.999, "the frame must have lit and shadowed texels"
    p.close()
    return dg.result()


def run_ao(ctx, case):
    import torch
    _, hr, _, _, synth, _ = _modules()
    sw, params = AO[case]
    wd, scale, band, dg = _setup(ctx, sw)
    p = _create(lambda: hr.RayTracedAO(ctx, W << scale, H << scale, scale, band=band), sw)
    p.params.exact = 0
    for k, v in params.items():
        setattr(p.params, k, v)
    zbp = synth.z_buffer_params()
    for f in range(FRAMES):
        fi = _inputs(hr, wd, f, scale, z_buffer_params=zbp)
        if sw.get("stages"):
            p.ray_trace(wd["gsc"], fi)
            p.temporal(fi)
            p.blur(fi, 0)
            p.blur(fi, 1)
        else:
            p.render(wd["gsc"], fi)
        torch.cuda.synchronize()
        dg.add("temporal", p.image(p.IMG_AO1 if f & 1 else p.IMG_AO0))
        dg.add("tiles", p.image(p.IMG_TILES), tiles=True)
        if sw.get("stages") or p.params.blur_radius != 4:   # the fused launch does not write the X image
            dg.add("blur0", p.image(p.IMG_BLUR0))
        dg.add("blur1", p.image(p.IMG_BLUR1))
        if scale:
            dg.add("upsample", p.output(hr.OUTPUT_UPSAMPLE), full=True)
    v = p.image(p.IMG_BLUR1)[slice(*dg.rows) if dg.rows else slice(None)].float().cpu().numpy()
    assert 0.05 < (v < 0.999).mean() < 0.999, "the frame must have occluded and unoccluded texels"
    p.close()
    return dg.result()


def run_reflections(ctx, case):
    import torch
    helpers, hr, api_gi, api_reflections, _, synth_env = _modules()
    sw, params = REFLECTIONS[case]
    wd, scale, band, dg = _setup(ctx, sw, mirror=True)
    FW, FH = W << scale, H << scale
    lo, hi = helpers.scene_data("sponza_small").bounds()
    if "env" not in _worlds:
        sky = synth_env.sky_cubemap(16)
        f16 = lambda a: torch.from_numpy(a).cuda().view(torch.float16)
        _worlds["env"] = api_gi.environment(f16(sky), f16(synth_env.prefiltered_chain(sky, 5)), 16, 5, f16(synth_env.brdf_lut(16)))
    env = _worlds["env"]
    ddgi = api_gi.DDGI(ctx, FW, FH, synth_env.ddgi_uniforms(lo, hi, probe_counts=(5, 3, 4), rays_per_probe=64, normal_bias=0.1))
    ddgi.params.exact = 0
    p = _create(lambda: api_reflections.RayTracedReflections(ctx, FW, FH, scale, band=band), sw)
    p.params.exact = 0
    for k, v in params.items():
        setattr(p.params, k, v)
    rng = np.random.RandomState(3)
    for f in range(FRAMES):
        fi_full = hr.frame_inputs(wd["gbs"][f], wd["gbs"][f - 1 if f else 0], wd["ubos"][f], f, f & 1, wd["sob"], wd["sr"])
        ddgi.render(wd["gsc"], fi_full, env, synth_env.random_orientation(rng))
        fi = _inputs(hr, wd, f, scale)
        p.set_camera_delta((-1.5, 0.0, 0.0) if f else (0.0, 0.0, 0.0))
        p.render(wd["gsc"], fi, env, ddgi)
        torch.cuda.synchronize()
        dg.add("ddgi", ddgi.output(), full=True)
        dg.add("temporal", p.image(p.IMG_COLOR1 if f & 1 else p.IMG_COLOR0))
        dg.add("tiles", p.image(p.IMG_TILES), tiles=True)
        dg.add("atrous0", p.image(p.IMG_ATROUS0))
        dg.add("atrous1", p.image(p.IMG_ATROUS1))
        if p.params.blur_as_input:
            dg.add("feedback", p.image(p.IMG_PREV))
        dg.add("output", p.output(hr.OUTPUT_ATROUS))
        if scale:
            dg.add("upsample", p.output(hr.OUTPUT_UPSAMPLE), full=True)
        if sw.get("stages"):
            for i in range(p.params.filter_iterations):
                p.atrous_iteration(fi, i)
                torch.cuda.synchronize()
                dg.add(f"iteration{i}", p.image(p.IMG_ATROUS0 if i & 1 else p.IMG_ATROUS1))
    tiles = p.image(p.IMG_TILES).cpu().numpy()
    assert 0.02 < tiles.mean() < 1.0, "the frame must have filtered and copied tiles"
    p.close(); ddgi.close()
    return dg.result()


RUNNERS = {"shadows": (run_shadows, SHADOWS), "ao": (run_ao, AO), "reflections": (run_reflections, REFLECTIONS)}


def _check(ctx, which, case):
    with open(FIXTURE) as fh:
        want = json.load(fh)[f"{which}/{case}"]
    got = RUNNERS[which][0](ctx, case)
    assert sorted(got) == sorted(want), f"{which}/{case}: stages {sorted(got)} against the fixture's {sorted(want)}"
    bad = [s for s in want if got[s] != want[s]]
    assert not bad, f"{which}/{case}: the bits of stage(s) {', '.join(bad)} differ from tests/golden/fast_filters.json"


@pytest.mark.parametrize("case", list(SHADOWS))
def test_shadows_chain_bits(hr, ctx, case):
    _check(ctx, "shadows", case)


@pytest.mark.parametrize("case", list(AO))
def test_ao_chain_bits(hr, ctx, case):
    _check(ctx, "ao", case)


@pytest.mark.parametrize("case", list(REFLECTIONS))
def test_reflections_chain_bits(hr, ctx, case):
    _check(ctx, "reflections", case)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_fast_filters.py --record   (rewrites tests/golden/fast_filters.json from the loaded library)")
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    from hybrid_rendering_amd import api
    api.lib()
    context = api.Context(0)
    recorded = {f"{which}/{case}": run(context, case) for which, (run, cases) in RUNNERS.items() for case in cases}
    with open(FIXTURE, "w") as fh:
        json.dump(recorded, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(recorded)} cases, {sum(len(v) for v in recorded.values())} digests -> {FIXTURE} (library: {api.LIB_PATH})")
