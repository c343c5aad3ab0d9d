"""The contract of include/hr_probe_vis.h restated in numpy — numpy only: no GPU, no library.  Every value is a float32 and every operation
is written in the order the contract gives, so the results equal csrc/probe_vis.hip's bit for bit.  The winner is found by brute force:
every pixel against every probe, the smallest accepted t, the first (smallest) index on a tie.

Reused rather than restated: dot3 and normalize3 (tests/env_reference.py, the fp32 forms), the octahedral fold, the saturating float -> int
conversion and the clamped bilinear fetch (tests/shading_reference.py: _oct_encode, _bilinear — dtype-generic, float32 in gives the device's
operations in the device's order).  world_pos_from_depth and mul_m4 had only float64 restatements (tests/reproject_cases.py unproject): their
fp32 forms are written out here, in device_math.h's order."""
import numpy as np

import env_reference as er
import shading_reference as sr

F = np.float32


def mul_m4(M, x, y, z, w):
    """column-major mat4 * vec4, rows summed left to right (device_math.h mul_m4); M: 16 float32"""
    M = np.asarray(M, F)
    return [((M[0 + r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w for r in range(4)]


def world_pos_from_depth(u, v, depth, vpi):
    one = np.ones_like(u)
    wp = mul_m4(vpi, u * F(2) - F(1), v * F(2) - F(1), depth * one, one)
    with np.errstate(all="ignore"):
        return np.stack([wp[0] / wp[3], wp[1] / wp[3], wp[2] / wp[3]], -1)


def pixel_dirs(ubo, w, h):
    """gb_pixel_dir at every pixel centre: [h][w][3]"""
    x = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    y = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    u, v = np.meshgrid(x, y)
    far = world_pos_from_depth(u.astype(F), v.astype(F), F(1), ubo["view_proj_inverse"])
    with np.errstate(all="ignore"):
        return er.normalize3(far - np.asarray(ubo["cam_pos"], F)[:3], F)


def probe_centres(grid):
    """[n][3] float32 in index order: grid_coord_to_position of probe_index_to_grid_coord"""
    nx, ny, nz = [int(c) for c in grid["probe_counts"]]
    p = np.arange(nx * ny * nz)
    g = np.stack([p % nx, (p % (nx * ny)) // nx, p // (nx * ny)], 1).astype(F)
    return np.asarray(grid["grid_step"], F) * g + np.asarray(grid["grid_start_position"], F)


def sphere_test(o, d, c, r):
    """the contract's test, broadcasting: (accepted, t)"""
    with np.errstate(all="ignore"):
        oc = o - c
        b = er.dot3(oc, d)
        q = oc - d * b[..., None]
        disc = F(r) * F(r) - er.dot3(q, q)
        hit = disc >= 0
        t = -b - np.sqrt(np.where(hit, disc, F(0)))
        return hit & (t > 0), t


def winners_of_rays(o, d, centres, radius):
    """o [3], d [m][3], centres [n][3] -> (t [m] float32, p [m], -1 where no probe is accepted, accepted count [m]): brute force over all probes"""
    o, d, centres = np.asarray(o, F), np.asarray(d, F), np.asarray(centres, F)
    tb, pb, nb = np.empty(len(d), F), np.empty(len(d), np.int64), np.empty(len(d), np.int64)
    for s in range(0, len(d), 512):
        ok, t = sphere_test(o, d[s:s + 512, None, :], centres[None], radius)
        t = np.where(ok, t, F(np.inf))
        p = t.argmin(1)                  # the first of equal minima: the smallest index
        tb[s:s + 512] = t[np.arange(t.shape[0]), p]
        pb[s:s + 512] = np.where(ok.any(1), p, -1)
        nb[s:s + 512] = ok.sum(1)
    return tb, pb, nb


def winners(ubo, grid, radius, w, h):
    t, p, n = winners_of_rays(np.asarray(ubo["cam_pos"], F)[:3], pixel_dirs(ubo, w, h).reshape(-1, 3), probe_centres(grid), radius)
    return t.reshape(h, w), p.reshape(h, w), n.reshape(h, w)


def texture_coord_from_direction(n, p, tw, th, side):
    """shading.h: normalises its argument (again), folds, places the probe's cell; n [m][3] float32, p [m] -> (u, v) float32"""
    with np.errstate(all="ignore"):
        z = (sr._oct_encode(er.normalize3(n, F)).astype(F) + F(1)) * F(0.5)
    per_row = (tw - 2) // (side + 2)
    col, row = (p % per_row).astype(F), (p // per_row).astype(F)
    pwb = F(side) + F(2)
    with np.errstate(all="ignore"):
        return (col * pwb + F(2)) / F(tw) + (z[:, 0] * F(side)) / F(tw), (row * pwb + F(2)) / F(th) + (z[:, 1] * F(side)) / F(th)


def h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(F)


def f2h(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, F).astype(np.float16).view(np.uint16)


def render(ubo, grid, irradiance, depth_atlas, radius, what, depth_in, color):
    """ubo: synth.UBO_DTYPE record; grid: synth_env.DDGI_DTYPE record; irradiance [H][W][4] / depth_atlas [H][W][2] fp16 bits; depth_in [h][w]
    float32; color [h][w][4] fp16 bits.  Returns dict(color, depth_out, probe_id, hit): the three outputs and the winner before the depth test."""
    h, w = depth_in.shape
    t, p, _ = winners(ubo, grid, radius, w, h)
    o = np.asarray(ubo["cam_pos"], F)[:3]
    d = pixel_dirs(ubo, w, h)
    has = p >= 0
    with np.errstate(all="ignore"):
        P = o + d * np.where(has, t, F(0))[..., None]
        clip = mul_m4(ubo["view_proj"], P[..., 0], P[..., 1], P[..., 2], np.ones_like(t))
        z = clip[2] / clip[3]
        drawn = has & (clip[3] > 0) & (z < depth_in)
    out = dict(color=color.copy(), depth_out=np.where(drawn, z, depth_in).astype(F), probe_id=np.where(drawn, p, -1).astype(np.int32), hit=np.where(has, p, -1))
    if not drawn.any():
        return out
    pd = p[drawn]
    with np.errstate(all="ignore"):
        n = er.normalize3(P[drawn] - probe_centres(grid)[pd], F)
    if what == 0:
        u, v = texture_coord_from_direction(n, pd, int(grid["irradiance_texture_width"]), int(grid["irradiance_texture_height"]), int(grid["irradiance_probe_side_length"]))
        rgb = sr._bilinear(h2f(irradiance)[..., :3], u, v)
    else:
        u, v = texture_coord_from_direction(n, pd, int(grid["depth_texture_width"]), int(grid["depth_texture_height"]), int(grid["depth_probe_side_length"]))
        with np.errstate(all="ignore"):
            g = sr._bilinear(h2f(depth_atlas), u, v)[:, 0] / F(grid["max_distance"])
        rgb = np.stack([g, g, g], 1)
    assert rgb.dtype == F
    out["color"][drawn] = np.concatenate([f2h(rgb), np.full((len(pd), 1), 0x3c00, np.uint16)], 1)
    return out
