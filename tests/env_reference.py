"""The numerical contract of include/hr_env.h restated in numpy — numpy only: no GPU, no oracle, no library.

With dtype = np.float32 every value is a float32 and every operation is written in the order the contract gives, so the results equal
csrc/env.hip's bit for bit; with dtype = np.float64 the same code is the sanity check of the contract itself (tests/test_env_host.py).
fp16 stores go through astype(np.float16) (round to nearest even).  Everything is vectorised over texels; the sums over samples keep the
contract's pairing: lane k adds i = k, k + 64, ... in increasing i from +0, then acc = acc + acc[idx ^ m] for m = 32 ... 1.  A sample the
contract skips adds +0 here, which leaves every partial sum's bits alone (a sum that starts at +0 is never -0)."""
import numpy as np

LANES = np.arange(64)


def bitreverse32(i):
    i = np.asarray(i, np.uint64)
    out = np.zeros_like(i)
    for b in range(32):
        out |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return out.astype(np.uint32)


def sample_table(n):
    """the contract's sample table by numpy's own cos / sin (the library's is compared with this one to 1 fp32 ulp)"""
    i = np.arange(n)
    xi1 = i.astype(np.float32) / np.float32(n)
    xi2 = bitreverse32(i).astype(np.float32) * np.float32(2.0 ** -32)
    phi = 2.0 * np.pi * xi2.astype(np.float64)
    return np.stack([xi1, np.cos(phi).astype(np.float32), np.sin(phi).astype(np.float32), np.zeros(n, np.float32)], -1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v, F):
    return v * (F(1) / np.sqrt(dot3(v, v)))[..., None]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def texel_dirs(s, F):
    """[6][s][s][3]: the unnormalised direction of every texel of a cubemap of size s"""
    t = F(2) * ((np.arange(s).astype(F) + F(0.5)) / F(s)) - F(1)
    u, v = np.meshgrid(t, t)          # u along x (columns), v along y (rows)
    one = np.ones_like(u)
    return np.stack([np.stack([one, -v, -u], -1), np.stack([-one, -v, u], -1), np.stack([u, one, v], -1),
                     np.stack([u, -one, -v], -1), np.stack([u, -v, one], -1), np.stack([-u, -v, -one], -1)]).astype(F)


def _texel_index(c, S, F):
    with np.errstate(invalid="ignore"):
        i = np.floor(c * F(S))
        i = np.where(np.isnan(i), 0, i)
        return np.clip(i, 0, S - 1).astype(np.int64)


def cube_fetch(sky_u16, d, F):
    """CubeMap::fetch (csrc/shading.h): NEAREST, x over y over z with >=; sky_u16 [6][S][S][4] fp16 bits, d [...][3] -> rgb [...][3]"""
    S = sky_u16.shape[1]
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    fx, fy = (ax >= ay) & (ax >= az), ay >= az
    face = np.where(fx, np.where(x >= 0, 0, 1), np.where(fy, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
    sc = np.where(fx, np.where(x >= 0, -z, z), np.where(fy, x, np.where(z >= 0, x, -x)))
    tc = np.where(fx, -y, np.where(fy, np.where(y >= 0, z, -z), -y))
    ma = np.where(fx, ax, np.where(fy, ay, az))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = F(0.5) * (sc / ma + F(1))
        t = F(0.5) * (tc / ma + F(1))
    ix, iy = _texel_index(s, S, F), _texel_index(t, S, F)
    return sky_u16.view(np.float16)[face, iy, ix, :3].astype(F)


def ggx_half(r, table, F):
    """Ht [n][3] for roughness r (a scalar of dtype F or an array broadcast against the table's rows)"""
    xi1, c, s = table[..., 0].astype(F), table[..., 1].astype(F), table[..., 2].astype(F)
    a = r * r
    a2 = a * a
    cos2 = (F(1) - xi1) / (F(1) + (a2 - F(1)) * xi1)
    ct = np.sqrt(cos2)
    st = np.sqrt(F(1) - ct * ct)
    return np.stack([st * c, st * s, ct], -1)


def wave_sum(contrib, F):
    """contrib [...][n], n a multiple of 64: the contract's sum over samples (per-lane sequential sums, then the xor butterfly)"""
    n = contrib.shape[-1]
    assert n % 64 == 0
    c = contrib.reshape(contrib.shape[:-1] + (n // 64, 64))
    acc = np.zeros(contrib.shape[:-1] + (64,), F)
    for j in range(n // 64):
        acc = acc + c[..., j, :]
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., LANES ^ m]
    assert acc.dtype == F
    return acc[..., 0]


def level_roughness(l, levels, F):
    return F(0) if levels == 1 else F(l) / F(levels - 1)


def prefiltered_chain(sky_u16, size, levels, table, F=np.float32):
    """the packed chain as fp16 bits, [texels][4]"""
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for l in range(levels):
            s = size >> l
            N = normalize3(texel_dirs(s, F), F)                                   # [6][s][s][3]
            texel = np.ones((6, s, s, 4), F)
            if l == 0:
                texel[..., :3] = cube_fetch(sky_u16, N, F)
            else:
                Ht = ggx_half(level_roughness(l, levels, F), table, F)          # [n][3]
                up = np.where((np.abs(N[..., 2]) < F(0.999))[..., None], np.array([0, 0, 1], F), np.array([1, 0, 0], F))
                T = normalize3(cross3(up, N), F)
                B = cross3(N, T)
                Nn, Tn, Bn = N[..., None, :], T[..., None, :], B[..., None, :]    # [6][s][s][1][3] against Ht [n][3]
                H = (Tn * Ht[:, 0:1] + Bn * Ht[:, 1:2]) + Nn * Ht[:, 2:3]
                L = H * (F(2) * dot3(Nn, H))[..., None] - Nn
                nl = dot3(Nn, L)                                                  # [6][s][s][n]
                on = nl > 0
                c = cube_fetch(sky_u16, L, F)
                w = wave_sum(np.where(on, nl, F(0)), F)
                for ch in range(3):
                    texel[..., ch] = wave_sum(np.where(on, c[..., ch] * nl, F(0)), F) / w
            assert texel.dtype == F
            out.append(texel.astype(np.float16).reshape(-1, 4))
    return np.ascontiguousarray(np.concatenate(out)).view(np.uint16)


def brdf_lut_values(lut, table, F=np.float32):
    """[lut][lut][2] in dtype F, before the fp16 store: rows = roughness, columns = N.V"""
    n = len(table)
    c = (np.arange(lut).astype(F) + F(0.5)) / F(lut)
    nv, r = c[None, :, None], c[:, None, None]                                    # [1][lut][1], [lut][1][1] against samples [n]
    V = (np.sqrt(F(1) - nv * nv), F(0), nv)
    k = (r * r) / F(2)
    H = ggx_half(r, table[None, None], F)                                         # [lut][1][n][3]
    vh = (V[0] * H[..., 0] + V[1] * H[..., 1]) + V[2] * H[..., 2]                 # [lut][lut][n]
    Lz = H[..., 2] * (F(2) * vh) - V[2]
    nl, nh = Lz, H[..., 2]
    on = nl > 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g1v = nv / (nv * (F(1) - k) + k)
        g1l = nl / (nl * (F(1) - k) + k)
        gv = ((g1v * g1l) * vh) / (nh * nv)
        t = F(1) - vh
        fc = ((t * t) * (t * t)) * t
        A = wave_sum(np.where(on, (F(1) - fc) * gv, F(0)), F) / F(n)
        B = wave_sum(np.where(on, fc * gv, F(0)), F) / F(n)
    out = np.stack([A, B], -1)
    assert out.dtype == F and out.shape == (lut, lut, 2)
    return out


def brdf_lut(lut, table, F=np.float32):
    """[lut][lut][2] fp16 bits"""
    return np.ascontiguousarray(brdf_lut_values(lut, table, F).astype(np.float16)).view(np.uint16)


def sh9(sky_u16, F=np.float32):
    """[9][4] in dtype F (rgb, .w = 0)"""
    S = sky_u16.shape[1]
    d = texel_dirs(S, F)
    r2 = dot3(d, d)
    wt = F(4) / (r2 * np.sqrt(r2))
    nrm = normalize3(d, F)
    rgb = cube_fetch(sky_u16, nrm, F)
    x, y, z = nrm[..., 0], nrm[..., 1], nrm[..., 2]
    basis = [np.full_like(x, F(0.282095)), F(-0.488603) * y, F(0.488603) * z, F(-0.488603) * x, (F(1.092548) * x) * y, (F(-1.092548) * y) * z,
             F(0.315392) * (((F(3) * z) * z) - F(1)), (F(-1.092548) * x) * z, F(0.546274) * (x * x - y * y)]
    terms = [rgb[..., c] * (b * wt) for b in basis for c in range(3)] + [wt]      # 28 x [6][S][S]
    pad = (-S) % 64
    rows = np.stack([wave_sum(np.pad(t, ((0, 0), (0, 0), (0, pad))), F) for t in terms], -1).reshape(6 * S, 28)
    total = np.zeros(28, F)
    for r in range(6 * S):
        total = total + rows[r]
    scale = (F(4) * F(3.14159265359)) / total[27]
    out = np.zeros((9, 4), F)
    out[:, :3] = (total[:27] * scale).reshape(9, 3)
    assert total.dtype == F and out.dtype == F
    return out


def chain_offsets(size, levels):
    """first texel of every level of the packed chain, and the total"""
    off = [0]
    for l in range(levels):
        off.append(off[-1] + 6 * (size >> l) ** 2)
    return off
