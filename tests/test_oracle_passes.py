"""Known-answer / property tests of the oracle's AO, DDGI and reflections restatements (CPU only)."""
import ctypes as C
import hashlib
import json

import numpy as np

import helpers
from hybrid_rendering_amd import synth, synth_env


def _quad_scene(tris, name="kat"):
    v = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return synth.SceneData(v, np.repeat(n[:, None], 3, 1).astype(np.float32), np.zeros(len(v), np.uint32), np.ones(len(v), np.uint32),
                           np.array([[0.8, 0.8, 0.8, 0.0, 0.02, 0, 0, 0]], np.float32), name)


FLOOR = [[(-500, 0, -500), (-500, 0, 500), (500, 0, 500)], [(-500, 0, -500), (500, 0, 500), (500, 0, -500)]]


def test_ao_open_plane_is_unoccluded_and_closed_room_is_occluded(oracle):
    sob, sr = synth.blue_noise_tables()
    cam = synth.Camera((0.0, 20.0, 60.0), (0.0, 0.0, 0.0), aspect=1.0)
    ubo = synth.make_ubo(cam, None, synth.sponza_light())
    # (a) a lone floor: every cosine-hemisphere ray escapes -> bit 1 for every non-sky pixel
    sc = oracle.Scene(_quad_scene(FLOOR))
    gb = sc.gbuffer(ubo, 64, 64)
    mask, rays = oracle.ao_ray_trace(sc, ubo, gb["depth"], gb["gb2"], sob, sr)
    bits, nonsky = helpers.unpack_mask(mask[0], 64, 64), gb["depth"] != 1.0
    assert nonsky.sum() > 500 and rays == nonsky.sum()
    assert np.array_equal(bits.astype(bool), nonsky)
    # (b) inside a closed 8-unit room every ray (length 7 > half-diagonal) is blocked... use a 4-unit room
    room = synth._Builder()
    room.box((-2, 0, -2), (2, 4, 2), 0, inward=True)
    rs = room.finish([[0.8, 0.8, 0.8, 0, 0.5, 0, 0, 0]], "room")
    sc2 = oracle.Scene(rs)
    cam2 = synth.Camera((0.0, 2.0, 1.5), (0.0, 1.0, -2.0), aspect=1.0, near=0.1, far=100.0)
    ubo2 = synth.make_ubo(cam2, None, synth.sponza_light())
    gb2 = sc2.gbuffer(ubo2, 48, 48)
    mask2, _ = oracle.ao_ray_trace(sc2, ubo2, gb2["depth"], gb2["gb2"], sob, sr, bias=0.05, ray_length=7.0)
    # (pixels within t_min = 0.01 of a second wall legitimately leak through it: allow a handful)
    assert (gb2["depth"] != 1.0).all() and int(helpers.unpack_mask(mask2[0], 48, 48).sum()) <= 8
    # temporal on frame 0: no history => output == this frame's bit, length 1; fully visible tiles need no blur
    out, ln, tiles = oracle.ao_temporal(ubo, mask, gb, gb, np.zeros((64, 64), np.uint16), np.zeros((64, 64), np.uint16))
    assert np.array_equal(oracle.f16(out)[nonsky], np.ones(nonsky.sum(), np.float32)) and (oracle.f16(ln)[nonsky] == 1.0).all()
    assert tiles.sum() == 0


def test_rng_matches_an_independent_xoroshiro64star(oracle):
    """random.glsl:11-56 re-implemented in Python integers."""
    M = 0xFFFFFFFF

    def rotl(x, k): return ((x << k) | (x >> (32 - k))) & M

    def hash_(s):
        s = ((s ^ 61) ^ (s >> 16)) & M; s = (s * 9) & M; s ^= s >> 4; s = (s * 0x27d4eb2d) & M; s ^= s >> 15
        return s

    def seq(ix, iy, frame, n):
        x, y = hash_(((ix << 16) | iy) & M), hash_(frame)
        def nxt():
            nonlocal x, y
            r = (x * 0x9e3779bb) & M
            y ^= x; x = rotl(x, 26) ^ y ^ ((y << 9) & M); y = rotl(y, 13)
            return r
        nxt()
        return [np.uint32(0x3f800000 | (nxt() >> 9)).view(np.float32) - np.float32(1.0) for _ in range(n)]

    out = (C.c_float * 6)()
    for ix, iy, fr in ((0, 0, 0), (255, 2047, 7), (13, 999, 123456)):
        oracle.lib().orc_rng_sequence(C.c_uint32(ix), C.c_uint32(iy), C.c_uint32(fr), 6, out)
        assert list(out) == [float(v) for v in seq(ix, iy, fr, 6)]
        assert all(0.0 <= v < 1.0 for v in out)


def test_spherical_fibonacci_and_gi_oct(oracle):
    L = oracle.lib()
    o3, e2, d3 = (C.c_float * 3)(), (C.c_float * 2)(), (C.c_float * 3)()
    pts = []
    for i in range(256):
        L.orc_spherical_fibonacci(C.c_float(i), C.c_float(256), o3)
        pts.append(list(o3))
    pts = np.array(pts)
    assert np.allclose(np.linalg.norm(pts, axis=1), 1.0, atol=2e-6)
    assert abs(pts.mean(0)).max() < 0.02                                        # well distributed over the sphere
    assert np.allclose(pts[:, 2], 1.0 - (2.0 * np.arange(256) + 1.0) / 256.0, atol=1e-6)
    rng = np.random.RandomState(0)
    for v in rng.normal(size=(300, 3)):
        v = (v / np.linalg.norm(v)).astype(np.float32)
        L.orc_gi_oct((C.c_float * 3)(*v), e2, d3)
        assert max(abs(e2[0]), abs(e2[1])) <= 1.0001 and np.allclose(d3[:], v, atol=3e-6)


def test_border_copy_formula_equals_the_reference_tables(oracle):
    """gi_border_update.glsl:35-143 — the oracle/kernels generate the copy table by formula.  The reference's two tables (depth probe
    16x16, irradiance probe 8x8) are held as the SHA-256 of json.dumps({"depth": [[sx, sy, dx, dy], ...], "irradiance": [...]}) in table
    order: the formula's tables must hash to it."""
    REF_TABLES_SHA256 = "3e773ced8103e11ad7debf8565b004d4ff3d911c67ff8409cb474f759d39270f"

    def gen(S):
        t = [(S + 1 - i, 1, i, 0) for i in range(1, S + 1)] + [(S + 1 - i, S, i, S + 1) for i in range(1, S + 1)]
        t += [(1, S + 1 - j, 0, j) for j in range(1, S + 1)] + [(S, S + 1 - j, S + 1, j) for j in range(1, S + 1)]
        return t + [(S, S, 0, 0), (1, S, S + 1, 0), (S, 1, 0, S + 1), (1, 1, S + 1, S + 1)]
    irr = gen(8)
    tables = json.dumps({"depth": [list(t) for t in gen(16)], "irradiance": [list(t) for t in irr]})
    assert hashlib.sha256(tables.encode()).hexdigest() == REF_TABLES_SHA256
    # and the oracle's in-place border update realises exactly that table on a probe filled with unique values
    from oracle import pyoracle_ddgi as od
    d = synth_env.ddgi_uniforms((0, 0, 0), (4, 4, 4), probe_counts=(1, 1, 1), rays_per_probe=8)
    atlas = np.zeros((12, 12, 4), np.uint16)
    atlas[2:10, 2:10, 0] = (np.arange(64, dtype=np.uint16) + 1).reshape(8, 8)
    od.border_update(d, False, atlas)
    for sx, sy, dx, dy in irr:
        assert atlas[1 + dy, 1 + dx, 0] == atlas[1 + sy, 1 + sx, 0] != 0


def test_probe_update_of_constant_radiance(oracle):
    """Every ray returns radiance c, distance r: irradiance texels -> 0.95*c, depth texels -> (r', r'^2)."""
    from oracle import pyoracle_ddgi as od
    d = synth_env.ddgi_uniforms((0, 0, 0), (4, 4, 4), probe_counts=(2, 1, 1), rays_per_probe=64)
    L, o3 = oracle.lib(), (C.c_float * 3)()
    dirs = []
    for i in range(64):
        L.orc_spherical_fibonacci(C.c_float(i), C.c_float(64), o3); dirs.append(list(o3))
    dirs = np.array(dirs, np.float32)
    rad = np.zeros((2, 64, 4), np.float16); rad[..., :3] = (0.5, 0.25, 1.0)
    dd = np.zeros((2, 64, 4), np.float16); dd[..., :3] = dirs; dd[..., 3] = 1.5
    irr0 = np.zeros((int(d["irradiance_texture_height"]), int(d["irradiance_texture_width"]), 4), np.uint16)
    dep0 = np.zeros((int(d["depth_texture_height"]), int(d["depth_texture_width"]), 2), np.uint16)
    irr = od.probe_update(d, False, True, rad.view(np.uint16), dd.view(np.uint16), irr0)
    dep = od.probe_update(d, True, True, rad.view(np.uint16), dd.view(np.uint16), dep0)
    assert np.allclose(oracle.f16(irr[2:10, 2:10, :3]), np.float32([0.5, 0.25, 1.0]) * 0.95, rtol=2e-3)
    assert (oracle.f16(irr[2:10, 2:10, 3]) == 1.0).all() and (irr[0] == 0).all()
    rp = min(float(d["max_distance"]), 1.5 - 0.01)
    assert np.allclose(oracle.f16(dep[2:18, 2:18, 0]), rp, rtol=2e-3) and np.allclose(oracle.f16(dep[2:18, 2:18, 1]), rp * rp, rtol=3e-3)


def test_reflection_rays_that_miss_return_the_sky(oracle):
    """rgen mirror branch + rmiss + nearest cube fetch: trace against an EMPTY scene, so every ray misses."""
    from oracle import pyoracle_ddgi as od, pyoracle_reflections as orf
    sob, sr = synth.blue_noise_tables()
    cam = synth.Camera((0.0, 30.0, 80.0), (0.0, 0.0, 0.0), aspect=1.0)
    ubo = synth.make_ubo(cam, None, synth.sponza_light())
    gscene = oracle.Scene(_quad_scene(FLOOR))
    gb = gscene.gbuffer(ubo, 32, 32)
    gb["gb3"][..., 0] = np.float16(0.02).view(np.uint16)                      # mirror regime
    empty = oracle.Scene(_quad_scene([[(1e6, 1e6, 1e6), (1e6 + 1, 1e6, 1e6), (1e6, 1e6 + 1, 1e6)]]))
    d = synth_env.ddgi_uniforms((-500, 0, -500), (500, 100, 500), probe_counts=(2, 2, 2), rays_per_probe=8)
    sky = synth_env.sky_cubemap(8)
    env = dict(sky=sky, prefiltered=synth_env.prefiltered_chain(sky, 4), pre_size=8, pre_levels=4, lut=synth_env.brdf_lut(8))
    irr = np.zeros((int(d["irradiance_texture_height"]), int(d["irradiance_texture_width"]), 4), np.uint16)
    dep = np.zeros((int(d["depth_texture_height"]), int(d["depth_texture_width"]), 2), np.uint16)
    tp = orf.TraceParams(0.5, 0.8, 0, 1, 1, 0.5, 0.5, 0.05)
    out, rays = orf.ray_trace(empty, ubo, d, gb, sob, sr, tp, env, irr, dep)
    nonsky = gb["depth"] != 1.0
    assert rays == nonsky.sum() > 100
    col, length = oracle.f16(out[..., :3]), oracle.f16(out[..., 3])
    assert (length == -1.0).all()
    skyf = sky.view(np.float16).astype(np.float32)
    # reflected ray of a floor pixel points up: it must land in the upper half of the cube map and be clamped at 0.7
    up_face_max = np.minimum(skyf[2, ..., :3].reshape(-1, 3).max(0), 0.7)
    assert (col[nonsky] <= 0.7003).all() and (col[nonsky][:, 2] > 0.3).all()
    assert (col[~nonsky] == 0).all() and np.all(col[nonsky].max(0) <= up_face_max + 0.71)
