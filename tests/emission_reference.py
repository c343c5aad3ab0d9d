"""The contract of include/hr_emission.h restated in float32 numpy (csrc/emission.h emission_at, bit for bit): every operation in np.float32 and in
the kernel's order, the texel divided by 255 in float32, REPEAT by modulo.  No GPU, no library."""
import numpy as np

F = np.float32


def sample_rgb(tex, tu, tv):
    """channels 0..2 of the pinned sampler (csrc/cutout.h sample_texture_channels): level 0, bilinear at uv * size - 0.5, REPEAT, UNORM8 = b / 255.
    Also returns the weights fx, fy (for the case file's own checks)."""
    h, w = tex.shape[0], tex.shape[1]
    tu, tv = np.asarray(tu, F), np.asarray(tv, F)
    px, py = tu * F(w) - F(0.5), tv * F(h) - F(0.5)
    fx0, fy0 = np.floor(px), np.floor(py)
    fx, fy = px - fx0, py - fy0
    ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)
    x0, x1, y0, y1 = ix % w, (ix + 1) % w, iy % h, (iy + 1) % h
    one = F(1.0)
    out = np.zeros(tu.shape + (3,), F)
    for c in range(3):
        ch = tex[..., c].astype(F)
        a, b, e, g = ch[y0, x0] / F(255.0), ch[y0, x1] / F(255.0), ch[y1, x0] / F(255.0), ch[y1, x1] / F(255.0)
        top, bot = a * (one - fx) + b * fx, e * (one - fx) + g * fx
        out[..., c] = top * (one - fy) + bot * fy
    return out, fx, fy


def hit_uv(uvs, q, u, v):
    """the hit shading's interpolation: tu = (uv0.x*b0 + uv1.x*b1) + uv2.x*b2 with b0 = 1 - u - v; (0, 0) without uvs"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    if uvs is None:
        return np.zeros_like(u), np.zeros_like(u)
    b0 = F(1.0) - u - v
    t = np.asarray(uvs, F)[q]
    return (t[:, 0, 0] * b0 + t[:, 1, 0] * u) + t[:, 2, 0] * v, (t[:, 0, 1] * b0 + t[:, 1, 1] * u) + t[:, 2, 1] * v


def emits(rgb, tex):
    """per material: its constant has a non-zero component or it has an emissive texture"""
    return (np.asarray(rgb, F) != 0).any(1) | (np.asarray(tex) >= 0)


def emission(tri_material, uvs, textures, rgb, tex, scale, q, u, v):
    """E [n][3] float32 and the select `on` [n] for hits on attribute triangles q (int array; < 0: a miss) with barycentrics u, v.
    tri_material / uvs: by attribute triangle; rgb [m][3], tex [m] (-1 none): the scene's emissive tables; textures: the scene's."""
    q = np.asarray(q, np.int64)
    u, v = np.asarray(u, F), np.asarray(v, F)
    rgb, tex = np.asarray(rgb, F), np.asarray(tex, np.int64)
    E, on = np.zeros((len(q), 3), F), np.zeros(len(q), bool)
    hit = np.flatnonzero(q >= 0)
    if not len(hit):
        return E, on
    mat = np.asarray(tri_material, np.int64)[q[hit]]
    on[hit] = emits(rgb, tex)[mat]
    Fc = rgb[mat].copy()
    tu, tv = hit_uv(uvs, q[hit], u[hit], v[hit])
    for t in np.unique(tex[mat]):
        if t < 0:
            continue
        k = tex[mat] == t
        Fc[k] = sample_rgb(textures[int(t)], tu[k], tv[k])[0]
    e = (F(scale) * Fc).astype(F)
    E[hit] = np.where(on[hit][:, None], e, F(0.0))
    return E, on


def fp16_bits(x):
    return np.asarray(x, F).astype(np.float16).view(np.uint16)


def ulp_distance16(a_bits, b_bits):
    """distance in fp16 ulps between finite values of the same sign class (non-negative radiance): the difference of the ordered bit patterns"""
    o = lambda b: np.where(b & 0x8000, -(b & 0x7fff).astype(np.int32), (b & 0x7fff).astype(np.int32))
    return np.abs(o(np.asarray(a_bits, np.uint16)) - o(np.asarray(b_bits, np.uint16)))
