"""A plain float64 restatement of the shading layer, written from the GLSL it ports (brdf.glsl, lighting.glsl, gi/gi_common.glsl, random.glsl,
scene_descriptor_set.glsl, reflections_ray_trace.rgen:78-105, gi_ray_trace.rgen:61-72) and from the samplers DESIGN.md §3 pins — NOT from the oracle's
or the device's sources.  Real pi, real 1e-4, numpy's sin / cos / pow, every operation in float64; the only fp32 facts kept are the pinned ones a
float64 evaluation cannot reproduce by itself: a float -> int conversion saturates at the int range (NaN -> 0).

reference(case) -> list of Check: the planes of one function, their float64 values, whether they are discrete (must be equal) or continuous, and
for continuous ones the natural magnitude `scale` of the quantity (the error unit of a plane is max(ulp32(|value|), ulp32(1) * scale): a component
of a unit vector is judged against the vector's length, a difference against its operands)."""
from dataclasses import dataclass

import numpy as np

import shading_cases as sc

PI = np.pi
EPS = 1e-4
ULP1 = 2.0 ** -23


@dataclass
class Check:
    function: str
    planes: list
    ref: np.ndarray          # [len(planes)][n] float64
    discrete: bool = False
    scale: object = 1.0      # scalar or [n]


def _f64(c):
    return c.inp.astype(np.float64)


def _norm(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _dot(a, b):
    return (a * b).sum(-1)


def _sat_int(x):
    """float -> int as the samplers mean it: saturating, NaN -> 0 (the result stays a float64 holding an integer)"""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), -2.0 ** 31, 2.0 ** 31 - 1))


def _h2f(a):
    return np.asarray(a, np.uint16).view(np.float16).astype(np.float64)


# ---- rng (random.glsl:11-56): integers, exact -------------------------------------------------------------------------------------------
def _rng(c):
    M = np.uint64(0xffffffff)
    u = lambda x: np.asarray(x, np.uint64) & M

    def hash_(s):
        s = u((s ^ np.uint64(61)) ^ (s >> np.uint64(16)))
        s = u(s * np.uint64(9))
        s = u(s ^ (s >> np.uint64(4)))
        s = u(s * np.uint64(0x27d4eb2d))
        return u(s ^ (s >> np.uint64(15)))
    rotl = lambda x, k: u((x << np.uint64(k)) | (x >> np.uint64(32 - k)))
    w = c.inp[:, 0:3].copy().view(np.uint32).astype(np.uint64)
    st = [hash_(u((w[:, 0] << np.uint64(16)) | w[:, 1])), hash_(w[:, 2])]

    def nxt():
        r = u(st[0] * np.uint64(0x9e3779bb))
        st[1] = st[1] ^ st[0]
        st[0] = rotl(st[0], 26) ^ st[1] ^ u(st[1] << np.uint64(9))
        st[1] = rotl(st[1], 13)
        return r
    nxt()
    out = []
    for _ in range(8):
        bits = (np.uint64(0x3f800000) | (nxt() >> np.uint64(9))).astype(np.uint32)
        out.append(bits.view(np.float32).astype(np.float64) - 1.0)
    return [Check("next_float", list(range(8)), np.array(out), discrete=True)]


# ---- cube maps (Vulkan face selection, NEAREST) -----------------------------------------------------------------------------
def _cube_fetch(d, S):
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    fx, fy = (ax >= ay) & (ax >= az), ay >= az
    face = np.where(fx, np.where(x >= 0, 0, 1), np.where(fy, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
    sc_ = np.where(fx, np.where(x >= 0, -z, z), np.where(fy, x, np.where(z >= 0, x, -x)))
    tc = np.where(fx, -y, np.where(fy, np.where(y >= 0, z, -z), -y))
    ma = np.where(fx, ax, np.where(fy, ay, az))
    with np.errstate(all="ignore"):
        s, t = 0.5 * (sc_ / ma + 1.0), 0.5 * (tc / ma + 1.0)
        ix, iy = np.clip(_sat_int(np.floor(s * S)), 0, S - 1), np.clip(_sat_int(np.floor(t * S)), 0, S - 1)
    return face.astype(np.float64), iy, ix


def _cube(c):
    v, T = _f64(c), c.tables
    f, iy, ix = _cube_fetch(v[:, 0:3], T["cube_size"])
    with np.errstate(all="ignore"):
        level = np.clip(_sat_int(np.floor(v[:, 3] + 0.5)), 0, T["pre_levels"] - 1)
    pf, piy, pix = np.zeros(len(v)), np.zeros(len(v)), np.zeros(len(v))
    for l in range(T["pre_levels"]):
        m = level == l
        if m.any():
            a, b, cc = _cube_fetch(v[m, 0:3], T["pre_size"] >> l)
            pf[m], piy[m], pix[m] = a + 8 * l, b, cc
    n = T["lut_size"]
    with np.errstate(all="ignore"):
        lx, ly = np.clip(_sat_int(np.floor(v[:, 4] * n)), 0, n - 1), np.clip(_sat_int(np.floor(v[:, 5] * n)), 0, n - 1)
    return [Check("CubeMap::fetch", [0, 1, 2], np.array([f, iy, ix]), discrete=True), Check("prefiltered_fetch", [3, 4, 5], np.array([pf, piy, pix]), discrete=True),
            Check("lut_fetch", [6, 7], np.array([lx, ly]), discrete=True)]


# ---- the RGBA8 sampler (bilinear at uv * size - 0.5, REPEAT, b / 255) and the alpha test -----------------------------------------------------
def _sample_texture(T, tex, u, v):
    out = np.zeros((4, len(u)))
    table, data = T["tex_table"], T["tex_data"].view(np.uint8).reshape(-1, 4).astype(np.float64) / 255.0
    for t in np.unique(tex):
        m = tex == t
        off, w, h = int(table[t][0]), int(table[t][1]), int(table[t][2])
        with np.errstate(all="ignore"):
            px, py = u[m] * w - 0.5, v[m] * h - 0.5
            fx, fy = px - np.floor(px), py - np.floor(py)
            x0, y0 = np.mod(_sat_int(np.floor(px)), w).astype(np.int64), np.mod(_sat_int(np.floor(py)), h).astype(np.int64)
        x1, y1 = (x0 + 1) % w, (y0 + 1) % h
        tx = lambda x, y: data[off + y * w + x].T
        with np.errstate(all="ignore"):
            out[:, m] = (tx(x0, y0) * (1 - fx) + tx(x1, y0) * fx) * (1 - fy) + (tx(x0, y1) * (1 - fx) + tx(x1, y1) * fx) * fy
    return out


def _texture(c):
    v, T = _f64(c), c.tables
    idx = lambda x, n: np.clip(_sat_int(x), 0, n - 1).astype(np.int64)
    rgba = _sample_texture(T, idx(v[:, 0], T["n_tex"]), v[:, 1], v[:, 2])
    q = idx(v[:, 3], T["n_attr"])
    tab, uvs = T["cutout_tab"], T["uvs"].astype(np.float64)
    b1, b2 = v[:, 4], v[:, 5]
    b0 = 1.0 - b1 - b2
    tu = uvs[q, 0, 0] * b0 + uvs[q, 1, 0] * b1 + uvs[q, 2, 0] * b2
    tv = uvs[q, 0, 1] * b0 + uvs[q, 1, 1] * b1 + uvs[q, 2, 1] * b2
    tex1 = tab[q, 0].astype(np.int64)
    alpha = _sample_texture(T, np.maximum(tex1 - 1, 0), tu, tv)[3]
    cutoff = tab[q, 1].copy().view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        accept = np.where(tex1 == 0, 1.0, np.where(alpha < cutoff, 0.0, 1.0))
    return [Check("sample_texture", [0, 1, 2, 3], rgba), Check("cutout_accept", [4], accept[None], discrete=True)]


# ---- brdf.glsl:36-142, deferred.frag:145-148 -----------------------------------------------------------------------------------------------
def _D(ndoth, alpha):
    a2 = alpha * alpha
    den = ndoth * ndoth * (a2 - 1.0) + 1.0
    return a2 / np.maximum(EPS, PI * den * den)


def _G1(r, nv):
    k = (r + 1) * (r + 1) / 8.0
    return nv / np.maximum(EPS, nv * (1 - k) + k)


def _F(f0, vh):
    return f0 + (1.0 - f0) * ((1.0 - vh) ** 5)[:, None]


def _spec(r, F, nh, nl, nv):
    return (_D(nh, r * r) * _G1(r, nl) * _G1(r, nv))[:, None] * F / np.maximum(EPS, 4.0 * nl * nv)[:, None]


def _brdf_terms(c):
    v = _f64(c)
    r, nh, nl, nv, vh = v[:, 18], v[:, 19], v[:, 20], v[:, 21], v[:, 22]
    with np.errstate(all="ignore"):
        F = _F(v[:, 12:15], vh)
        return [Check("D_ggx", [0], _D(nh, r * r)[None], scale=1 / EPS), Check("G_schlick_ggx", [1], (_G1(r, nl) * _G1(r, nv))[None], scale=1 / EPS),
                Check("F_schlick", [2, 3, 4], F.T), Check("evaluate_specular_brdf", [5, 6, 7], _spec(r, F, nh, nl, nv).T, scale=1 / EPS)]


def _nanmax0(a):
    """GLSL max(a, 0.0): max(x, y) = x < y ? y : x keeps a NaN first operand"""
    with np.errstate(all="ignore"):
        return np.where(a < 0.0, 0.0, a)


def _brdf_uber(c):
    v = _f64(c)
    N, Wo, Wi, Wh, F0, dc, r = v[:, 0:3], v[:, 3:6], v[:, 6:9], v[:, 9:12], v[:, 12:15], v[:, 15:18], v[:, 18]
    with np.errstate(all="ignore"):
        nl, nv, nh, vh = _nanmax0(_dot(N, Wi)), _nanmax0(_dot(N, Wo)), _nanmax0(_dot(N, Wh)), _nanmax0(_dot(Wi, Wh))
        F = _F(F0, vh)
        uber = (1.0 - F) * (dc / PI) + _spec(r, F, nh, nl, nv)
        ct = v[:, 21]
        fsr = F0 + (np.maximum(1.0 - r[:, None], F0) - F0) * (_nanmax0(1.0 - ct) ** 5)[:, None]
    return [Check("evaluate_uber_brdf", [0, 1, 2], uber.T, scale=1 / EPS), Check("fresnel_schlick_roughness", [3, 4, 5], fsr.T)]


# ---- brdf.glsl:8-32, :96-112, reflections_ray_trace.rgen:78-105 ----------------------------------------------------------------------------------
def _rotation(n):
    ref = np.where((np.abs(n[:, 1]) > np.float64(np.float32(0.99)))[:, None], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0])
    x = _norm(np.cross(ref, n))
    return x, np.cross(n, x)


def _apply(x, y, n, t):
    return _norm(x * t[:, 0:1] + y * t[:, 1:2] + n * t[:, 2:3])


def _lobes(c):
    v = _f64(c)
    n, r0, r1, rough = v[:, 0:3], v[:, 3], v[:, 4], v[:, 5]
    with np.errstate(all="ignore"):
        x, y = _rotation(n)
        rx, ry = np.maximum(np.float64(np.float32(0.00001)), r0), np.maximum(np.float64(np.float32(0.00001)), r1)
        phi = 2.0 * PI * ry
        cos_lobe = _apply(x, y, n, np.stack([np.sqrt(1 - rx) * np.cos(phi), np.sqrt(1 - rx) * np.sin(phi), np.sqrt(rx)], 1))
        # importance_sample_ggx(E = (r0, r1), N, Roughness = rough)
        m2 = rough ** 4
        ct = np.sqrt((1 - r1) / (1 + (m2 - 1) * r1))
        st = np.sqrt(1 - ct * ct)
        phi = 2.0 * PI * r0
        up = np.where((np.abs(n[:, 2]) < np.float64(np.float32(0.999)))[:, None], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
        tg = _norm(np.cross(up, n))
        ggx = _norm(tg * (np.cos(phi) * st)[:, None] + np.cross(n, tg) * (np.sin(phi) * st)[:, None] + n * ct[:, None])
        # sample_specular_ggx_lobe(n, alpha = rough, Xi = (r0, r1))
        ct = np.sqrt((1 - r1) / (1 + (rough * rough - 1) * r1))
        st = np.sqrt(1 - ct * ct)
        spec = _apply(x, y, n, np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1))
    return [Check("sample_cosine_lobe_n", [0, 1, 2], cos_lobe.T), Check("sample_cosine_lobe", [3, 4, 5], cos_lobe.T), Check("importance_sample_ggx", [6, 7, 8], ggx.T),
            Check("sample_specular_ggx_lobe", [9, 10, 11], spec.T)]


# ---- lighting.glsl:6-111 -------------------------------------------------------------------------------------------------------------------
def _smoothstep(e0, e1, x):
    """GLSL leaves smoothstep undefined for edge0 >= edge1; the pinned meaning (device_math.h smoothstep1, docs/TOLERANCE.md) is the formula with a
    clamp that takes a NaN quotient (an empty cone with the angle exactly on it: 0 / 0) to 0"""
    with np.errstate(all="ignore"):
        q = (x - e0) / (e1 - e0)
        t = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, 1.0))
        return t * t * (3 - 2 * t)


def _lights(c, soft):
    v = _f64(c)
    P, N, Wo, rx, ry = v[:, 0:3], v[:, 3:6], v[:, 6:9], v[:, 9], v[:, 10]
    ldir, inten, lpos, lrad = v[:, 11:14], v[:, 14], v[:, 15:18], v[:, 18]
    typ, co, ci = np.trunc(v[:, 19]), v[:, 20], v[:, 21]
    colour = np.asarray(c.tables["light"], np.float64)[8:11]
    with np.errstate(all="ignore"):
        to_light = lpos - P
        dist = np.sqrt(_dot(to_light, to_light))
        direc = typ == 0
        light_dir = np.where(direc[:, None], ldir, _norm(to_light))
        t_max = np.where(direc, 10000.0, dist)
        if soft:
            radius = np.where(direc, lrad, lrad / dist)
            tg = _norm(np.cross(light_dir, [0.0, 1.0, 0.0]))
            bt = _norm(np.cross(tg, light_dir))
            pr, pa = radius * np.sqrt(rx), ry * 2 * PI
            Wi = _norm(light_dir + tg * (pr * np.cos(pa))[:, None] + bt * (pr * np.sin(pa))[:, None])
        else:
            Wi = light_dir
        att = np.where(direc, 1.0, np.where(typ == 1, 1.0 / (dist * dist), _smoothstep(co, ci, _dot(Wi, ldir)) / (dist * dist)))
        att = att * np.clip(_dot(N, Wi), 0.0, 1.0)
        scale_att = np.where(direc, 1.0, 1.0 / (dist * dist))
        scale_att = np.where(np.isfinite(scale_att), scale_att, 1.0)
        if soft:
            return [Check("fetch_light_shadow.Wi", [0, 1, 2], Wi.T), Check("fetch_light_shadow.t_max", [3], t_max[None]), Check("fetch_light_shadow.attenuation", [4], att[None], scale=scale_att)]
        Li = colour[None, :] * inten[:, None]
        Wh = _norm(Wo + Wi)
        return [Check("fetch_light_hard.Li", [0, 1, 2], Li.T), Check("fetch_light_hard.Wi", [3, 4, 5], Wi.T), Check("fetch_light_hard.Wh", [6, 7, 8], Wh.T),
                Check("fetch_light_hard.t_max", [9], t_max[None]), Check("fetch_light_hard.attenuation", [10], att[None], scale=scale_att)]


# ---- gi_common.glsl:39-184, gi_ray_trace.rgen:61-72 ---------------------------------------------------------------------------------------------
def _snz(k):
    return np.where(k >= 0, 1.0, -1.0)


def _oct_encode(v):
    with np.errstate(all="ignore"):
        r = v[:, 0:2] * (1.0 / np.abs(v).sum(1))[:, None]
        folded = (1.0 - np.abs(r[:, ::-1])) * _snz(r)
        return np.where((v[:, 2] < 0)[:, None], folded, r)


def _oct_decode(o):
    z = 1.0 - np.abs(o[:, 0]) - np.abs(o[:, 1])
    xy = np.where((z < 0)[:, None], (1.0 - np.abs(o[:, ::-1])) * _snz(o), o)
    return _norm(np.concatenate([xy, z[:, None]], 1))


def _uniforms(T):
    d = T["ddgi"]
    f = d.view(np.float32).astype(np.float64)
    return dict(start=f[0:3], step=f[3:6], counts=d[6:9].astype(np.int64), bias=f[12], energy=f[13], iside=int(d[14]), iw=int(d[15]), ih=int(d[16]), dside=int(d[17]),
                dw=int(d[18]), dh=int(d[19]), vis=int(d[21]))


def _gi_oct(c):
    v, U = _f64(c), _uniforms(c.tables)
    nx, ny, nz = U["counts"]
    idx = np.clip(_sat_int(v[:, 5]), 0, nx * ny * nz - 1).astype(np.int64)
    g = np.stack([idx % nx, (idx % (nx * ny)) // nx, idx // (nx * ny)], 1)
    i, n = v[:, 6], v[:, 7]
    with np.errstate(all="ignore"):
        phi_m1 = np.float64(np.float32(np.sqrt(np.float32(5)) * np.float32(0.5) + np.float32(0.5))) - 1.0      # PHI is an fp32 constant in the shader
        a = i * phi_m1
        phi = 2 * PI * (a - np.floor(a))
        ct = 1.0 - (2 * i + 1) * (1.0 / n)
        st = np.sqrt(np.clip(1 - ct * ct, 0.0, 1.0))
        fib = np.stack([np.cos(phi) * st, np.sin(phi) * st, ct], 1)
        # 2 pi frac(i * (PHI - 1)): the fraction of a product as large as i loses log2(i) bits before the sine sees it
        fib_scale = np.maximum(1.0, np.abs(i))
    return [Check("gi_oct_encode", [0, 1], _oct_encode(v[:, 0:3]).T), Check("gi_oct_decode", [2, 3, 4], _oct_decode(v[:, 3:5]).T),
            Check("probe_location", [5, 6, 7], (U["step"] * g + U["start"]).T, scale=np.abs(U["start"]).max() + np.abs(U["step"] * U["counts"]).max()),
            Check("spherical_fibonacci", [8, 9, 10], fib.T, scale=np.where(np.isfinite(fib_scale), fib_scale, 1.0))]


def _tex_coord(dirn, col, row, tw, th, side):
    with np.errstate(all="ignore"):
        z = (_oct_encode(_norm(dirn)) + 1.0) * 0.5
        pwb = side + 2.0
        return np.stack([(col * pwb + 2.0) / tw + z[:, 0] * side / tw, (row * pwb + 2.0) / th + z[:, 1] * side / th], 1)


def _gi_coords(c):
    v = _f64(c)
    tw, th, side, col, row = [_sat_int(v[:, k]) for k in (4, 5, 6, 7, 8)]
    uv = _tex_coord(v[:, 0:3], col, row, tw, th, side)
    inr = ((tw >= 1e-6) & (tw <= 3e5) & (th >= 1e-6) & (th <= 3e5)).astype(np.float64)
    return [Check("texture_coord_from_direction", [0, 1], uv.T), Check("texture_coord_from_cell.generic", [2, 3], uv.T), Check("texture_coord_from_cell.inrange", [4, 5], uv.T),
            Check("atlas_div_inrange", [6], inr[None], discrete=True)]


# ---- DDGI atlases (bilinear, clamp to edge; ddgi.cpp:478,499) and gi_common.glsl:188-320 ----------------------------------------------------------
def _bilinear(img, u, v):
    h, w = img.shape[:2]
    with np.errstate(all="ignore"):
        x, y = u * w - 0.5, v * h - 0.5
        fx, fy = x - np.floor(x), y - np.floor(y)
        x0, y0 = _sat_int(np.floor(x)), _sat_int(np.floor(y))
    cl = lambda a, n: np.clip(a, 0, n - 1).astype(np.int64)
    x1, y1 = cl(np.minimum(x0, 2.0 ** 31 - 2) + 1, w), cl(np.minimum(y0, 2.0 ** 31 - 2) + 1, h)
    x0, y0 = cl(x0, w), cl(y0, h)
    fx, fy = fx[:, None], fy[:, None]
    with np.errstate(all="ignore"):
        return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


def _gather(c):
    v, T, U = _f64(c), c.tables, _uniforms(c.tables)
    irr = _h2f(T["irradiance"]).reshape(U["ih"], U["iw"], 4)[..., :3]
    dep = _h2f(T["depth"]).reshape(U["dh"], U["dw"], 2)
    P, N, Wo = v[:, 2:5], v[:, 5:8], v[:, 8:11]
    cnt = U["counts"]
    with np.errstate(all="ignore"):
        base = np.clip(_sat_int((P - U["start"]) / U["step"]), 0, cnt - 1)
        alpha = np.clip((P - (U["step"] * base + U["start"])) / U["step"], 0.0, 1.0)
        s_irr, s_w = np.zeros((len(v), 3)), np.zeros(len(v))
        for i in range(8):
            off = np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])
            g = np.clip(base + off, 0, cnt - 1)
            col, row = g[:, 0] + g[:, 1] * cnt[0], g[:, 2]
            ppos = U["step"] * g + U["start"]
            p2p = P - ppos + (N + 3.0 * Wo) * U["bias"]
            dirn = _norm(-p2p)
            tri = np.where(off[None, :] == 1, alpha, 1.0 - alpha)
            t = (_dot(_norm(ppos - P), N) + 1.0) * 0.5
            t = np.where(EPS < t, t, EPS)                      # max(0.0001, t) with the specification's NaN rule
            w = t * t + 0.2
            if U["vis"] == 1:
                mm = _bilinear(dep, *_tex_coord(-dirn, col, row, U["dw"], U["dh"], U["dside"]).T)
                dist = np.sqrt(_dot(p2p, p2p))
                mean, var = mm[:, 0], np.abs(mm[:, 0] ** 2 - mm[:, 1])
                dm = np.where(dist - mean < 0, 0.0, dist - mean)
                che = var / (var + dm * dm)
                che = np.where(che ** 3 < 0, 0.0, che ** 3)
                w = w * np.where(dist <= mean, 1.0, che)
            w = np.where(1e-6 < w, w, 1e-6)
            pi_ = _bilinear(irr, *_tex_coord(_norm(N), col, row, U["iw"], U["ih"], U["iside"]).T)
            w = np.where(w < 0.2, w * (w * w * (1.0 / 0.04)), w)
            w = w * (tri[:, 0] * tri[:, 1] * tri[:, 2])
            s_irr += w[:, None] * np.sqrt(pi_)
            s_w += w
        net = s_irr / s_w[:, None]
        net = np.where(np.isnan(net), 0.5, net)
        out = 0.5 * PI * (net * net * U["energy"])
    top = float(irr.max())
    return [Check("atlas_bilinear_rgb", [0, 1, 2], _bilinear(irr, v[:, 0], v[:, 1]).T, scale=top), Check("atlas_bilinear_rg", [3, 4], _bilinear(dep, v[:, 0], v[:, 1]).T, scale=float(np.abs(dep).max()) + 1e-30),
            Check("sample_irradiance_net", [5, 6, 7], net.T, scale=np.sqrt(top)), Check("sample_irradiance", [8, 9, 10], out.T, scale=top * U["energy"] * PI / 2)]


# ---- scene_descriptor_set.glsl:133-220 ---------------------------------------------------------------------------------------------------------
def _surface(c):
    v, T = _f64(c), c.tables
    q = np.clip(_sat_int(v[:, 0]), 0, T["n_tris"] - 1).astype(np.int64)
    b1, b2 = v[:, 1], v[:, 2]
    b0 = 1.0 - b1 - b2
    flags = _sat_int(v[:, 3]).astype(np.int64)
    has_n, inst, textured, has_t = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0
    lerp = lambda a: a[q, 0] * b0[:, None] + a[q, 1] * b1[:, None] + a[q, 2] * b2[:, None]
    pos, nrm, tan, uvs = [T[k].astype(np.float64) for k in ("positions", "normals", "tangents", "tri_uvs")]
    M = T["inst_m"].astype(np.float64).reshape(4, 4).T            # column-major
    with np.errstate(all="ignore"):
        P = lerp(pos)
        P = np.where(inst[:, None], P @ M[:3, :3].T + M[:3, 3], P)
        n = np.where(has_n[:, None], lerp(nrm), np.cross(pos[q, 1] - pos[q, 0], pos[q, 2] - pos[q, 0]))
        xf = lambda a: np.where(inst[:, None], _norm(_norm(a) @ M[:3, :3].T), _norm(_norm(a)))
        Nn = xf(n)
        mat = T["tri_material"][q].astype(np.int64)
        mats, mt = T["materials"].astype(np.float64), T["mat_tex"]
        albedo, metallic, rough = mats[mat, 0:3].copy(), mats[mat, 3].copy(), np.maximum(mats[mat, 4], np.float64(np.float32(0.1)))
        uv = lerp(uvs)
        for m in range(T["n_mats"]):
            sel = textured & (mat == m)
            if not sel.any():
                continue
            smp = lambda t: _sample_texture(T, np.full(int(sel.sum()), t), uv[sel, 0], uv[sel, 1])
            if mt[m][0] >= 0:
                albedo[sel] = smp(mt[m][0])[:3].T
            if mt[m][2] >= 0:
                rough[sel] = np.maximum(smp(mt[m][2])[mt[m][4] & 3], np.float64(np.float32(0.1)))
            if mt[m][3] >= 0:
                metallic[sel] = smp(mt[m][3])[mt[m][5] & 3]
            if mt[m][1] >= 0:
                tg = np.where(has_t[sel][:, None], lerp(tan)[sel], [1.0, 0.0, 0.0])
                Tt = _norm(np.where(inst[sel][:, None], _norm(_norm(tg) @ M[:3, :3].T), _norm(_norm(tg))))
                tn = _norm(smp(mt[m][1])[:3].T * 2.0 - 1.0)
                Nn[sel] = _norm(Tt * tn[:, 0:1] + Tt * tn[:, 1:2] + _norm(Nn[sel]) * tn[:, 2:3])      # TBN = (T, T, N): the hit shaders pass the tangent twice
    big = float(np.abs(pos).max() * np.abs(M).max() * 3 + np.abs(M).max())
    return [Check("surface_from.P", [0, 1, 2], P.T, scale=big), Check("surface_from.N", [3, 4, 5], Nn.T), Check("surface_from.albedo", [6, 7, 8], albedo.T),
            Check("surface_from.roughness", [9], rough[None]), Check("surface_from.metallic", [10], metallic[None])]


_REF = {sc.RNG: _rng, sc.CUBE: _cube, sc.TEXTURE: _texture, sc.BRDF_TERMS: _brdf_terms, sc.BRDF_UBER: _brdf_uber, sc.LOBES: _lobes, sc.LIGHT_HARD: lambda c: _lights(c, False),
        sc.LIGHT_SHADOW: lambda c: _lights(c, True), sc.GI_OCT: _gi_oct, sc.GI_COORDS: _gi_coords, sc.GATHER: _gather, sc.SURFACE: _surface}


def reference(case):
    return _REF[case.mode](case)


def ulp32(x):
    """the fp32 unit in the last place at |x| (float64 in, float64 out); the smallest normal's for anything below it"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    a = np.where(np.isfinite(a), a, 2.0 ** 127)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def error_units(out, chk):
    """|oracle - float64| per element in units of max(ulp32(|float64|), ulp32(1) * scale), the worst plane of the function; NaN where either side
    is not finite (those elements are compared by class)"""
    o = np.asarray(out, np.float64)[chk.planes]
    unit = np.maximum(ulp32(chk.ref), ULP1 * np.asarray(chk.scale, np.float64))
    with np.errstate(all="ignore"):
        e = np.abs(o - chk.ref) / unit
    e = np.where(np.isfinite(o) & np.isfinite(chk.ref), e, np.nan)
    return e


def classes(x):
    """NaN / +inf / -inf / finite"""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 3)))
