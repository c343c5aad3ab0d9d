"""Shared test fixtures: seeded synthetic frames built with the oracle's CPU G-buffer synthesiser."""
from __future__ import annotations

import functools

import numpy as np

from hybrid_rendering_amd import synth


@functools.lru_cache(maxsize=8)
def scene_data(name: str):
    if name == "cornell":
        return synth.cornell32()
    if name == "sponza_small":
        return synth.sponza_like(0.25)
    if name == "sponza":
        return synth.sponza_like(1.0)
    if name == "sponza_hard":            # bench.py --tier hard: ~2.5 M triangles, layered fabric and foliage cards
        return synth.sponza_like(1.0, tier="hard")
    if name == "sponza_hard_small":
        return synth.sponza_like(0.5, tier="hard")
    if name.startswith("one_triangle"):
        return one_triangle_scene(int(name[len("one_triangle_x"):]) if name.startswith("one_triangle_x") else 1)
    raise KeyError(name)


def one_triangle_scene(copies: int = 1):
    """degenerate scene: ONE triangle in the middle of the Cornell set-up (the BVH root is a leaf), optionally `copies` times over
    (coincident duplicates with their own mesh ids: equal t, the tie rule decides)"""
    import dataclasses
    base = synth.cornell32()
    lo, hi = base.bounds()
    c, e = (lo + hi) * 0.5, (hi - lo) * 0.35
    tri = np.array([[[c[0] - e[0], c[1] - e[1], c[2]], [c[0] + e[0], c[1] - e[1], c[2] + 0.2 * e[2]], [c[0], c[1] + e[1], c[2] - 0.1 * e[2]]]], np.float32)
    n = np.cross(tri[0, 1] - tri[0, 0], tri[0, 2] - tri[0, 0])
    n = (n / np.linalg.norm(n)).astype(np.float32)
    return dataclasses.replace(base, verts=np.repeat(tri, copies, 0), normals=np.repeat(np.broadcast_to(n, (1, 3, 3)).copy(), copies, 0),
                               tri_material=np.zeros(copies, np.uint32), tri_mesh_id=np.arange(1, copies + 1, dtype=np.uint32),
                               uvs=None, tangents=None, material_textures=None, textures=None, name=f"one_triangle_x{copies}")


def _cornell_setup(name: str) -> bool:
    return name == "cornell" or name.startswith("one_triangle")


def cameras(name: str, aspect: float, n_frames: int, dolly: float):
    if _cornell_setup(name):
        base = synth.cornell_camera(aspect)
        cams = []
        for f in range(n_frames):
            e = np.array(base.eye) + np.array([0.6, 0.2, -1.0]) * dolly * f
            cams.append(synth.Camera(tuple(e), base.target, fov=base.fov, aspect=aspect))
        return cams
    return [synth.sponza_camera(aspect, frame=f, dolly=dolly) for f in range(n_frames)]


def light_for(name: str, kind: str = "default"):
    if _cornell_setup(name):
        return synth.cornell_light(hard=(kind != "soft"))
    if kind == "grazing":
        return synth.sponza_hard_light()
    if kind == "point":
        return synth.make_light(synth.LIGHT_POINT, position=(100.0, 300.0, 20.0), radius=4.0, intensity=50000.0)
    if kind == "spot":
        return synth.make_light(synth.LIGHT_SPOT, direction_to_light=(0.2, 1.0, 0.1), position=(60.0, 330.0, 30.0), radius=3.0,
                                intensity=50000.0, cone_inner_deg=25.0, cone_outer_deg=40.0)
    return synth.sponza_light()


def make_frames(oracle, oscene, name, w, h, n_frames=3, dolly=0.0, light_kind="default", scale_mips=0):
    """List of dicts(ubo, gb (numpy G-buffer at (w,h)), mips...) for consecutive frames."""
    cams = cameras(name, w / h, n_frames, dolly)
    light = light_for(name, light_kind)
    frames = []
    for f in range(n_frames):
        ubo = synth.make_ubo(cams[f], cams[f - 1] if f > 0 else None, light)
        gb = oscene.gbuffer(ubo, w, h)
        fr = dict(ubo=ubo, gb=gb)
        if scale_mips:
            fr["mips"] = [gb] + [nearest_mip(gb, s) for s in range(1, scale_mips + 1)]
        frames.append(fr)
    return frames


def nearest_mip(gb, level):
    """Point-sampled mip (g_buffer.cpp:240-243 VK_FILTER_NEAREST): keep texel (x << level, y << level)."""
    s = 1 << level
    h, w = gb["depth"].shape
    hh, ww = h >> level, w >> level
    return {k: np.ascontiguousarray(v[:hh * s:s, :ww * s:s]) for k, v in gb.items()}


def to_cuda(gb):
    import torch
    out = {}
    for k, v in gb.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        if t.dtype == torch.uint16:
            t = t.view(torch.float16)
        out[k] = t.cuda()
    return out


def bits16(t):
    """cuda fp16 tensor -> numpy uint16 bit patterns."""
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def unpack_mask(mask, w, h):
    bits = np.zeros((((h + 3) // 4) * 4, ((w + 7) // 8) * 8), np.uint8)
    for ly in range(4):
        for lx in range(8):
            bits[ly::4, lx::8] = (mask >> np.uint32(ly * 8 + lx)) & 1
    return bits[:h, :w]


def fuzz_configs(seed: int, n: int, hard: bool = False):
    """The random configurations of tools/fuzz_tolerance.py, as a generator of dicts — ONE place for the draws, so that a sequence a fuzz
    campaign found can be named (seed, trial) in a test (tests/test_gpu_tolerance.py FUZZ_SEQUENCES) and replayed by tools/fuzz_one.py."""
    rng = np.random.RandomState(seed)
    for trial in range(n):
        name = str(rng.choice(["sponza_hard_small", "sponza_hard_small", "sponza_small"] if hard else ["cornell", "sponza_small"]))
        # large enough that 0.1 % of the texels is a population, not two pixels
        W, H = int(rng.randint(160, 360)), int(rng.randint(120, 220))
        light = str(rng.choice(["default", "point", "spot"] + (["grazing", "grazing"] if hard else [])) if name != "cornell" else rng.choice(["default", "soft"]))
        dolly = float(rng.uniform(0.2, 2.5))
        scale = int(rng.choice([0, 1, 1, 2]))
        sp = ap = rp = None
        if trial % 2:
            sp = dict(alpha=float(rng.uniform(0.005, 0.3)), moments_alpha=float(rng.uniform(0.05, 0.5)), phi_visibility=float(rng.uniform(1, 20)),
                      phi_normal=float(rng.choice([8.0, 32.0, 64.0, 12.5])), sigma_depth=float(rng.uniform(0.3, 3)), power=float(rng.choice([0.0, 1.2, 2.0])),
                      radius=int(rng.choice([1, 2])), filter_iterations=int(rng.choice([1, 3, 5])), feedback_iteration=int(rng.choice([0, 1])))
            ap = dict(blur_radius=int(rng.choice([2, 4, 6])), alpha=float(rng.uniform(0.005, 0.3)), ray_length=float(rng.uniform(5, 60)))
            rp = dict(alpha=float(rng.uniform(0.005, 0.3)), moments_alpha=float(rng.uniform(0.05, 0.5)), phi_color=float(rng.uniform(1, 20)),
                      phi_normal=float(rng.choice([32.0, 8.0, 12.5])), sigma_depth=float(rng.uniform(0.3, 3)), radius=int(rng.choice([1, 2])),
                      filter_iterations=int(rng.choice([1, 3, 5])), feedback_iteration=int(rng.choice([0, 1])))
        ao_spp = int(rng.randint(1, 5))
        yield dict(trial=trial, name=name, W=W, H=H, light=light, dolly=dolly, scale=scale, shadows=sp, ao=ap, reflections=rp, ao_spp=ao_spp)


def fuzz_config(seed: int, trial: int, hard: bool = False):
    for c in fuzz_configs(seed, trial + 1, hard):
        pass
    return c


def _is_nan_bits(b):
    """NaN test on fp16 (uint16) or fp32 (uint32) bit patterns: exponent all ones and a non-zero mantissa, whatever the sign."""
    if b.dtype == np.uint16:
        return ((b & 0x7c00) == 0x7c00) & ((b & 0x03ff) != 0)
    return ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)


def assert_bits_equal_nan(got, ref, what):
    """got / ref: uint16 (fp16) or uint32 (fp32) bit patterns.  Bit-identical, except that two NaNs count as equal whatever their sign and
    payload (GLSL and HIP leave a NaN's payload unspecified).  +0 / -0, +-inf and every finite value must match bit for bit."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.dtype in (np.uint16, np.uint32), (what, got.dtype, ref.dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    both_nan = _is_nan_bits(got) & _is_nan_bits(ref)
    bad = (got != ref) & ~both_nan
    if bad.any():
        fl = np.float16 if got.dtype == np.uint16 else np.float32
        w = np.argwhere(bad)[:8]
        idx = tuple(w.T)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ (NaN == NaN); first (index): {w.tolist()} "
                             f"got {got[idx].view(fl).tolist()} ({[hex(int(v)) for v in got[idx]]}) "
                             f"ref {ref[idx].view(fl).tolist()} ({[hex(int(v)) for v in ref[idx]]})")
