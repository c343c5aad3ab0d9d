"""Adversarial G-buffers for the history reprojection (numpy only: no GPU, no oracle) — the counterpart of ray_cases.py for
reprojection.glsl:115-328 (csrc/reproject.h, Reproj<> in csrc/denoise_fast_common.h, oracle/orc_reproject.h).

craft(gb_h, gb_c, ubo_c) takes two consecutive rendered G-buffers (dicts gb1 / gb2 / gb3 / depth as oracle.Scene.gbuffer returns them) and the
current frame's UBO and returns rewritten copies (H, C) and an `info` dict.  Frame H is the history side — the caller passes it UNCHANGED as frame
C's `prev` — frame C the current side.  Every rewritten word is a finite, valid G-buffer value; |mv| <= 2 image extents; mesh ids are integers <= 2048.

Rewritten pixels stand on a "wall": one NDC depth and the normal facing the camera, so that a history tap's plane distance is ~0 and its cos^2 ~1
wherever a motion vector points — the MESH ID alone then decides a tap, except where a family puts one threshold under it.  Families (one
horizontal stripe of frame C each; A has a second stripe at the bottom, because an fp16 motion vector only resolves a target position from nearby):
  A shifts       hfx / hfy = (float)x + mv * extent on the listed positions around both borders of each axis, and the corners combined
  B tap subsets  4x4 "cells" of frame H whose ids match the current pixel on each subset of the 2x2 footprint, on each single texel of the
                 fallback's reach, on none; interior cells and cells straddling each border (what lies outside cannot match: those cases merge)
  C sumw         the reachable (fx, fy, subset) whose fp32 sum of weights, in the oracle's order, lies closest to 0.01f from either side
  D plane        integer shift, the tap's depth on an ulp ladder over the float64 crossing of |dot(cur_pos - hist_pos, n)| = 5; dense and sparse
  E normal       integer shift, the tap's oct code from a search for |cos^2 - 0.1| <= 1e-5; dense and sparse
  F sky          depth 1.0 at the current pixel, under some taps, under all taps
  G (reflections_variant) mirror roughness everywhere, curvature exactly 0 / non-zero in a checkerboard
info: family [h, w] uint8 (FAMILY), case [h, w] int32, and per family the arrays the self-checks and the GPU test's messages need."""
import numpy as np

F32 = np.float32
FAMILY = dict(none=0, A=1, B=2, C=3, D=4, E=5, F=6)
BG_ID = 7                      # the wall's mesh id
D_BASE, E_BASE, CELL_BASE = 64, 96, 128
LADDER = np.array(list(range(-16, 17)) + [-256, -64, -32, 32, 64, 256], np.int64)
SUBSETS = list(range(1, 16))   # bit s = tap s of the 2x2 footprint (s & 1: +x, s >> 1: +y)


def f16bits(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def f16val(b):
    return np.asarray(b, np.uint16).view(np.float16).astype(np.float64)


def targets(ext):
    """the issue's positions for an axis of `ext` texels, as fp32"""
    e = float(ext)
    t = [-2, -1.75, -1.25, -1, -0.75, -0.5, -0.25, -2.0 ** -10, 0, 0.25, float(np.nextafter(F32(0.5), F32(0))), 0.5,
         e - 1.5, e - 1, e - 0.5, e - 2.0 ** -10, e, e + 0.5]
    return np.array(t, F32)


def hist_coord(x, mv_bits, ext):
    """the kernel's hfx: (float)x + mv * extent, every operation fp32"""
    mv = np.asarray(mv_bits, np.uint16).view(np.float16).astype(F32)
    return (np.asarray(x, F32) + (mv * F32(ext)).astype(F32)).astype(F32)


def zone(hf):
    """the decisions a coordinate takes part in: ivec2() truncation, floor, the non-reflection passes' nearest texel"""
    hf = np.asarray(hf, F32)
    return np.stack([np.trunc(hf).astype(np.int64), np.floor(hf).astype(np.int64), np.trunc((hf + F32(0.5)).astype(F32)).astype(np.int64)], -1)


def aim(x, target, ext):
    """fp16 motion vector (bits) nearest to (target - x) / ext, and the coordinate it really gives"""
    mv = f16bits((np.asarray(target, np.float64) - np.asarray(x, np.float64)) / float(ext))
    return mv, hist_coord(x, mv, ext)


def integer_shift(ext):
    """smallest k > 0 with k / ext an fp16 value (the shift is then exactly k texels); 0 if none below ext / 4"""
    for k in range(1, max(ext // 4, 1)):
        if float(np.float16(k / ext)) * ext == k:
            return k
    return 0


def unproject(u, v, d, vpi):
    """float64 restatement of world_position_from_depth (common.glsl:169-184); vpi: the UBO's column-major view_proj_inverse"""
    M = np.asarray(vpi, np.float64).reshape(4, 4).T
    ndc = np.stack(np.broadcast_arrays(np.asarray(u, np.float64) * 2 - 1, np.asarray(v, np.float64) * 2 - 1, np.asarray(d, np.float64), 1.0), -1)
    p = ndc @ M.T
    return p[..., :3] / p[..., 3:4]


def oct_decode(ex, ey):
    """float64 octohedral_to_direction (common.glsl:150-156)"""
    ex, ey = np.asarray(ex, np.float64), np.asarray(ey, np.float64)
    z = 1.0 - np.abs(ex) - np.abs(ey)
    sx, sy = np.where(ex >= 0, 1.0, -1.0), np.where(ey >= 0, 1.0, -1.0)
    nx, ny = np.where(z < 0, (1 - np.abs(ey)) * sx, ex), np.where(z < 0, (1 - np.abs(ex)) * sy, ey)
    v = np.stack([nx, ny, z], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def oct_encode(n):
    n = np.asarray(n, np.float64)
    p = n[..., :2] / np.abs(n).sum(-1, keepdims=True)
    if n[..., 2] <= 0:
        p = (1 - np.abs(p[..., ::-1])) * np.where(p >= 0, 1.0, -1.0)
    return f16bits(p)


def normal_candidates(cur_code, tol=1e-5):
    """fp16 oct codes (x bits, y bits) with |dot(cur, n)^2 - 0.1| <= tol in float64, and the signed distances, sorted by |distance|.
    For every fp16 y the quadratic dot(cur, a + x b)^2 = 0.1 |a + x b|^2 of the upper hemisphere's two x half planes is solved and the fp16
    neighbours of its roots are evaluated."""
    c = oct_decode(*f16val(cur_code))
    yb = np.concatenate([np.arange(0x0400, 0x3c00, dtype=np.uint16), np.arange(0x8400, 0xbc00, dtype=np.uint16)])   # normal fp16 values in (-1, 1)
    y = f16val(yb)
    out_x, out_y = [], []
    for sx in (1.0, -1.0):
        a = np.stack([np.zeros_like(y), y, 1 - np.abs(y)], -1)
        b = np.array([1.0, 0.0, -sx])
        ca, cb, aa, ab, bb = a @ c, float(b @ c), (a * a).sum(-1), a @ b, 2.0
        qa, qb, qc = cb * cb - 0.1 * bb, 2 * (ca * cb - 0.1 * ab), ca * ca - 0.1 * aa
        disc = qb * qb - 4 * qa * qc
        ok = disc >= 0
        for sign in (1.0, -1.0):
            r = (-qb + sign * np.sqrt(np.where(ok, disc, 0.0))) / (2 * qa)
            good = ok & (r * sx > 2.0 ** -14) & (np.abs(r) + np.abs(y) <= 1.0)
            rb = f16bits(np.where(good, r, 0.5))[good].astype(np.int32)
            for k in range(-2, 3):
                out_x.append((rb + k).astype(np.uint16)); out_y.append(yb[good])
    xb, yb = np.concatenate(out_x), np.concatenate(out_y)
    key = np.unique(xb.astype(np.uint32) << 16 | yb)
    xb, yb = (key >> 16).astype(np.uint16), (key & 0xffff).astype(np.uint16)
    fin = np.isfinite(f16val(xb)) & (np.abs(f16val(xb)) <= 1.0)
    xb, yb = xb[fin], yb[fin]
    dist = (oct_decode(f16val(xb), f16val(yb)) @ c) ** 2 - 0.1
    keep = np.abs(dist) <= tol
    order = np.argsort(np.abs(dist[keep]), kind="stable")
    return xb[keep][order], yb[keep][order], dist[keep][order]


def weights32(fx, fy):
    fx, fy = np.asarray(fx, F32), np.asarray(fy, F32)
    one = F32(1)
    return [((one - fx) * (one - fy)).astype(F32), (fx * (one - fy)).astype(F32), ((one - fx) * fy).astype(F32), (fx * fy).astype(F32)]


def sumw32(fx, fy, subset):
    """the oracle's sum: sumw = 0; sumw += wgt[s] for the valid taps in order, every operation fp32"""
    w = weights32(fx, fy)
    s = np.zeros(np.broadcast(fx, fy).shape, F32)
    for k in range(4):
        if subset >> k & 1:
            s = (s + w[k]).astype(F32)
    return s


def ulps_from(x, ref):
    return np.asarray(x, F32).view(np.int32).astype(np.int64) - int(np.asarray(ref, F32).view(np.int32))


def stripes(h):
    """rows [r0, r1) of frame C per family; rows 0-2 and the last row stay rendered; no stripe starts on a multiple of 8"""
    share = [("A", 0.08), ("B", 0.13), ("C", 0.09), ("D", 0.25), ("E", 0.25), ("F", 0.09), ("A2", 0.11)]
    rows, r, avail = {}, 3, h - 4
    for i, (name, s) in enumerate(share):
        if r % 8 == 0:
            r += 1
        r1 = h - 1 if i == len(share) - 1 else min(h - 1, 3 + int(round(avail * sum(q for _, q in share[:i + 1]))))
        rows[name] = (r, max(r1, r + 1))
        r = rows[name][1]
    return rows


def cell_patterns():
    """(name, 4x4 bool: which texels of the cell carry the matching id).  The footprint is the cell's texels [1..2] x [1..2]."""
    pats = []
    for s in SUBSETS:
        m = np.zeros((4, 4), bool)
        for k in range(4):
            if s >> k & 1:
                m[1 + (k >> 1), 1 + (k & 1)] = True
        pats.append((f"subset{s:04b}", m))
    for j in range(4):
        for i in range(4):
            if not (1 <= i <= 2 and 1 <= j <= 2):
                m = np.zeros((4, 4), bool); m[j, i] = True
                pats.append((f"ring{i}{j}", m))
    pats.append(("none", np.zeros((4, 4), bool)))
    return pats


SHIFTS = [(0.0, 0.0), (0.25, 0.25), (0.5, 0.75), (0.75, 0.5)]
POOLS = ("interior", "left", "right", "top", "bottom")


def cell_inside(pool):
    """which texels of a 4x4 cell of that pool lie inside the image (a border cell straddles its border two texels deep)"""
    return {"interior": np.ones((4, 4), bool), "left": np.arange(4)[None, :] >= 2, "right": np.arange(4)[None, :] < 2,
            "top": np.arange(4)[:, None] >= 2, "bottom": np.arange(4)[:, None] < 2}[pool] & np.ones((4, 4), bool)


def craft(gb_h, gb_c, ubo_c, seed=0):
    H = {k: v.copy() for k, v in gb_h.items()}
    C = {k: v.copy() for k, v in gb_c.items()}
    h, w = C["depth"].shape
    vpi = np.asarray(ubo_c["view_proj_inverse"], np.float32)
    cam = np.asarray(ubo_c["cam_pos"], np.float64)[:3]
    fwd = unproject(0.5, 0.5, 0.5, vpi) - cam
    fwd /= np.linalg.norm(fwd)
    up = unproject(0.5, 0.0, 0.5, vpi) - unproject(0.5, 1.0, 0.5, vpi)
    up -= fwd * (up @ fwd); up /= np.linalg.norm(up)
    # the wall: about one world unit per texel (a one-texel step then moves a position by far less than PLANE_DISTANCE), not behind the scene's median depth
    span = np.linalg.norm(unproject(0.5, 0.0, 0.5, vpi) - unproject(0.5, 1.0, 0.5, vpi)) / np.linalg.norm(unproject(0.5, 0.5, 0.5, vpi) - cam)
    z_of = lambda d: (unproject(0.5, 0.5, d, vpi) - cam) @ fwd
    lo_d, hi_d = np.float64(0.0), np.float64(1.0)
    geo = gb_c["depth"][gb_c["depth"] != 1.0]
    z_wall = min(h / span, float(z_of(np.median(geo)))) if geo.size else h / span
    for _ in range(60):
        mid = 0.5 * (lo_d + hi_d)
        lo_d, hi_d = (mid, hi_d) if z_of(mid) < z_wall else (lo_d, mid)
    d0 = F32(lo_d)
    d_far = np.nextafter(F32(1), F32(0))
    n0 = oct_encode(-fwd)
    clipz = lambda d: f16bits(np.asarray(d, np.float64) * z_of(np.asarray(d, np.float64)))   # GB3.w: clip-space z, as the G-buffer pass stores it

    def wall(G, ys, xs, mesh=BG_ID, depth=None, normal=None):
        d = d0 if depth is None else depth
        G["depth"][ys, xs] = d
        G["gb2"][ys, xs, 0], G["gb2"][ys, xs, 1] = (n0 if normal is None else normal)
        G["gb2"][ys, xs, 2:] = 0
        G["gb3"][ys, xs, 2] = f16bits(mesh)
        G["gb3"][ys, xs, 3] = clipz(d)

    rows = stripes(h)
    family, case = np.zeros((h, w), np.uint8), np.full((h, w), -1, np.int32)
    wall(H, slice(3, h - 1), slice(None))
    a_cols = w // 4
    for sl in (slice(0, a_cols), slice(w - a_cols, w)):       # family A's landing zones along the top and bottom borders
        wall(H, slice(0, 3), sl); wall(H, slice(h - 1, h), sl)
    for name, (r0, r1) in rows.items():
        wall(C, slice(r0, r1), slice(None))
    info = dict(rows=rows, d0=float(d0), size=(w, h))

    def set_pixel(y, x, fam, cs, mvx=0, mvy=0, mesh=BG_ID, depth=None, normal=None):
        wall(C, y, x, mesh, depth, normal)
        C["gb2"][y, x, 2], C["gb2"][y, x, 3] = mvx, mvy
        family[y, x], case[y, x] = FAMILY[fam], cs

    # ---------------------------------------------------------------------------------------------------------------- A
    tx, ty = targets(w), targets(h)
    A = []
    allx, ally = np.arange(w), np.arange(h)

    def best(t, cand, ext, n):
        mv, got = aim(cand, t, ext)
        same = (zone(got) == zone(t)).all(-1)
        order = np.lexsort((np.abs(cand - float(t)), np.abs(got.astype(np.float64) - float(t)), ~same))
        return [(int(cand[i]), mv[i], got[i]) for i in order[:n]]
    a_rows = list(range(*rows["A"])) + list(range(*rows["A2"]))
    used = set()
    for i, t in enumerate(tx):                                 # x targets: any column, a row of either A stripe, no vertical motion
        k = 0
        for x, mv, got in best(t, allx, w, 40):
            y = next((yy for yy in a_rows[(i + 5 * k) % len(a_rows):] + a_rows if (yy, x) not in used), None)
            if y is None or k == 6:
                continue
            used.add((y, x))
            set_pixel(y, x, "A", i, mvx=mv, mesh=0 if k == 5 else BG_ID)       # the last copy carries mesh id 0: what an outside texel reads as
            A.append((y, x, 0, i, got, F32(y)))
            k += 1
    ycols = [x for x in list(range(1, a_cols - 2)) + list(range(w - a_cols + 1, w - 2))]
    a_ys = np.array(a_rows)
    for i, t in enumerate(ty):                                 # y targets: a row of an A stripe, a column above / below which frame H is wall
        for k, (y, mv, got) in enumerate(best(t, a_ys, h, 4)):
            x = next(xx for xx in ycols[(7 * i + 3 * k) % len(ycols):] + ycols if (y, xx) not in used)
            used.add((y, x))
            set_pixel(y, x, "A", 100 + i, mvy=mv, mesh=0 if k == 3 else BG_ID)
            A.append((y, x, 1, i, F32(x), got))
    corner_t = lambda e: ([F32(-1.25), F32(-0.75)], [F32(e - 1.5), F32(e - 0.5)])
    for cy, ys_t in enumerate(corner_t(h)):                    # the four corners: both coordinates off their borders at once
        for cx, xs_t in enumerate(corner_t(w)):
            for j, (t_x, t_y) in enumerate([(a, b) for a in xs_t for b in ys_t]):
                y, mvy, goty = best(t_y, a_ys, h, 1)[0]
                cand = np.array([xx for xx in allx if (y, xx) not in used])
                x, mvx, gotx = best(t_x, cand, w, 1)[0]
                used.add((y, x))
                set_pixel(y, x, "A", 200 + 16 * cy + 8 * cx + j, mvx=mvx, mvy=mvy)
                A.append((y, x, 2, 2 * cy + cx, gotx, goty))
    info["A"] = np.array(A, dtype=[("y", int), ("x", int), ("axis", int), ("target", int), ("hfx", F32), ("hfy", F32)])

    # ---------------------------------------------------------------------------------------------------------------- cells of frame H
    pats = cell_patterns()
    interior_rows = [r for fam in ("B", "C", "F") for r in range(rows[fam][0] + 1, rows[fam][1] - 4, 4)]
    pools = dict(interior=[(x, y) for y in interior_rows for x in range(4, w - 8, 4)],
                 left=[(-2, y) for y in range(rows["B"][0] + 1, rows["A2"][0] - 5, 4)], right=[(w - 2, y) for y in range(rows["B"][0] + 1, rows["A2"][0] - 5, 4)],
                 top=[(x, -2) for x in range(a_cols + 2, w - a_cols - 6, 4)], bottom=[(x, h - 2) for x in range(a_cols + 2, w - a_cols - 6, 4)])
    n_cells = [0]

    def place(pool, match, depth=None):
        """write a cell into frame H; returns (x of footprint tap 0, y of it, matching id)"""
        cx, cy = pools[pool].pop(0)
        mid = CELL_BASE + 2 * (n_cells[0] % 900); n_cells[0] += 1
        for j in range(4):
            for i in range(4):
                x, y = cx + i, cy + j
                if 0 <= x < w and 0 <= y < h:
                    wall(H, y, x, mid if match[j, i] else mid + 1, None if depth is None else depth[j, i])
        return cx + 1, cy + 1, mid
    inside = cell_inside

    # ---------------------------------------------------------------------------------------------------------------- B
    b_px = [(y, x) for y in range(*rows["B"]) for x in range(w)]
    rng = np.random.RandomState(seed)
    rng.shuffle(b_px)
    B, subset_cells = [], {}
    for pool in ("interior", "left", "right", "top", "bottom"):
        seen = set()
        for ci, (name, m) in enumerate(pats):
            mm = m & inside(pool)
            key = mm.tobytes()
            if key in seen or not pools[pool]:     # what lies outside the image cannot match: the case is another one's twin there
                continue
            seen.add(key)
            bx, by, mid = place(pool, mm)
            if pool == "interior" and name.startswith("subset"):
                subset_cells[int(name[6:], 2)] = (bx, by, mid)
            for si, (sx, sy) in enumerate(SHIFTS):
                y, x = b_px.pop()
                mvx, gx = aim(x, bx + sx, w)
                mvy, gy = aim(y, by + sy, h)
                cs = 1000 * ("interior", "left", "right", "top", "bottom").index(pool) + 10 * ci + si
                set_pixel(y, x, "B", cs, mvx=mvx, mvy=mvy, mesh=mid)
                B.append((y, x, cs, gx, gy))
    info["B"] = np.array(B, dtype=[("y", int), ("x", int), ("case", int), ("hfx", F32), ("hfy", F32)])
    info["B_cases"] = {1000 * p + 10 * ci: f"{pool}/{name}" for p, pool in enumerate(("interior", "left", "right", "top", "bottom")) for ci, (name, _) in enumerate(pats)}

    # ---------------------------------------------------------------------------------------------------------------- C
    c_rows = np.arange(*rows["C"])
    c_cols = np.arange(8, w - 8, max(1, (w - 16) // 48))[:48]
    codes = np.arange(-48, 49)
    ref = F32(0.01)
    cands = []
    for s in SUBSETS:
        bx, by, mid = subset_cells[s]
        # the lattice: fp16 motion vectors around the one that points at the cell, from each candidate column / row
        mvx0 = f16bits((bx + 0.5 - c_cols) / w).astype(np.int32)[:, None] + codes[None, :]
        mvy0 = f16bits((by + 0.5 - c_rows) / h).astype(np.int32)[:, None] + codes[None, :]
        with np.errstate(all="ignore"):      # codes stepped across zero are NaN patterns: they match no cell
            hx, hy = hist_coord(c_cols[:, None], mvx0.astype(np.uint16), w), hist_coord(c_rows[:, None], mvy0.astype(np.uint16), h)
        okx, oky = np.trunc(hx) == bx, np.trunc(hy) == by
        fx, fy = (hx - np.floor(hx)).astype(F32)[okx], (hy - np.floor(hy)).astype(F32)[oky]
        ix, iy = np.argwhere(okx), np.argwhere(oky)
        sw = sumw32(fx[:, None], fy[None, :], s)
        u = ulps_from(sw, ref)
        flat = np.argsort(np.abs(u), axis=None, kind="stable")[:600]
        for f in flat:
            a, b = divmod(int(f), sw.shape[1])
            cands.append((abs(int(u[a, b])), int(u[a, b]), s, int(c_rows[iy[b, 0]]), int(c_cols[ix[a, 0]]), int(mvx0[ix[a, 0], ix[a, 1]]), int(mvy0[iy[b, 0], iy[b, 1]]), float(sw[a, b]), mid))
    cands.sort()
    Cc, taken, n_side = [], set(), {True: 0, False: 0}
    for _, u, s, y, x, mvx, mvy, sw, mid in cands:
        below = u < 0
        if (y, x) in taken or n_side[below] >= 64:
            continue
        taken.add((y, x)); n_side[below] += 1
        set_pixel(y, x, "C", 16 * len(Cc) + s, mvx=np.uint16(mvx), mvy=np.uint16(mvy), mesh=mid)
        Cc.append((y, x, s, sw, u))
    info["C"] = np.array(Cc, dtype=[("y", int), ("x", int), ("subset", int), ("sumw", F32), ("ulps", int)])

    # ---------------------------------------------------------------------------------------------------------------- D, E: layouts
    sx = integer_shift(w)
    mvx_int = f16bits(sx / w)
    assert hist_coord(10, mvx_int, w) == 10 + sx

    def layouts(fam):
        r0, r1 = rows[fam]
        ntx = (w + 7) // 8
        x_ok = lambda x: 4 <= x < w - 4 and 3 <= x + sx < w - 3
        dense, sparse = [], []
        for t_y in range(r0 // 8, (r1 + 7) // 8):
            whole = t_y * 8 >= r0 and t_y * 8 + 8 <= r1
            for t_x in range(ntx):
                if whole and t_x < ntx // 2 and all(x_ok(t_x * 8 + i) for i in range(8)):
                    dense += [(t_y * 8 + j, t_x * 8 + i, t_x) for j in range(8) for i in range(8)]
                elif not (whole and t_x < ntx // 2):
                    y, x = t_y * 8 + (5 * t_x + 3 * t_y) % 8, t_x * 8 + (3 * t_x + 5 * t_y) % 8
                    if r0 <= y < r1 and x_ok(x):
                        sparse.append((y, x, t_x))
        return dense, sparse
    pid = lambda base, y, x: base + (x & 3) + 4 * (y & 3)      # 16 ids: no two texels of a 4x4 neighbourhood share one

    # ---------------------------------------------------------------------------------------------------------------- D
    tilt = [1.0, 0.3, 0.1]       # cosine between the current normal and the view axis: the flatter, the finer one ulp of depth moves the plane distance
    d_normals = [oct_encode(-fwd * c + up * np.sqrt(1 - c * c)) for c in tilt]
    D = []
    for lay, px in enumerate(layouts("D")):
        if not px:
            continue
        ys, xs = np.array([p[0] for p in px]), np.array([p[1] for p in px])
        k = np.arange(len(px))
        lad, cls, side = LADDER[k % len(LADDER)], (k // len(LADDER)) % 3, np.where((k // len(LADDER)) // 3 % 2 == 0, 1.0, -1.0)
        ncode = np.array(d_normals)[cls]
        n = oct_decode(f16val(ncode[:, 0]), f16val(ncode[:, 1]))
        tu, tv = ((xs.astype(F32) + F32(0.5)) / F32(w)).astype(F32), ((ys.astype(F32) + F32(0.5)) / F32(h)).astype(F32)
        htu = (tu + f16val(mvx_int).astype(F32)).astype(F32)
        cur = unproject(tu, tv, d0, vpi)
        g = lambda d: ((cur - unproject(htu, tv, d, vpi)) * n).sum(-1)
        lo, hi = np.full(len(px), 1e-3), np.full(len(px), 1.0)
        inc = g(hi) > g(lo)
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            up_ = (g(mid) < 5.0 * side) == inc
            lo, hi = np.where(up_, mid, lo), np.where(up_, hi, mid)
        good = (lo > 2e-3) & (hi < 1.0 - 1e-9)
        depth = (lo.astype(F32).view(np.int32) + lad.astype(np.int32)).view(F32)
        for i in np.nonzero(good & (depth < 1.0))[0]:
            y, x = int(ys[i]), int(xs[i])
            m = pid(D_BASE, y, x + sx)
            wall(H, y, x + sx, m, depth[i], ncode[i])
            set_pixel(y, x, "D", 100000 * lay + 1000 * int(cls[i]) + int(lad[i]) + 300, mvx=mvx_int, mesh=m, normal=ncode[i])
            D.append((y, x, lay, int(lad[i]), int(cls[i])))
    info["D"] = np.array(D, dtype=[("y", int), ("x", int), ("sparse", int), ("ulp", int), ("tilt", int)])

    # ---------------------------------------------------------------------------------------------------------------- E
    e_normals = [oct_encode(-fwd), oct_encode(-fwd * 0.8 + up * 0.6), oct_encode(-fwd * 0.6 - up * 0.8)]
    e_cands = [normal_candidates(c) for c in e_normals]
    E, nxt = [], [[0, 0, 0], [0, 0, 0]]
    for lay, px in enumerate(layouts("E")):
        for y, x, t_x in px:
            j = t_x % 3
            xb, yb, dist = e_cands[j]
            i = nxt[lay][j] % len(xb); nxt[lay][j] += 1
            m = pid(E_BASE, y, x + sx)
            wall(H, y, x + sx, m, None, (xb[i], yb[i]))
            set_pixel(y, x, "E", 100000 * lay + 10000 * j + i, mvx=mvx_int, mesh=m, normal=e_normals[j])
            E.append((y, x, lay, j, dist[i]))
    info["E"] = np.array(E, dtype=[("y", int), ("x", int), ("sparse", int), ("normal", int), ("dist", float)])
    info["E_pool"] = [len(c[0]) for c in e_cands]

    # ---------------------------------------------------------------------------------------------------------------- F
    f_px = [(y, x) for y in range(*rows["F"]) for x in range(2, w - 2)]
    rng.shuffle(f_px)
    Fs = []
    fi = 0
    for far in (True, False):
        for s in (15, 1, 6, 8):
            if not pools["interior"]:
                break
            dep = np.full((4, 4), d_far if far else d0, F32)
            for k in range(4):
                if s >> k & 1:
                    dep[1 + (k >> 1), 1 + (k & 1)] = 1.0
            bx, by, mid = place("interior", np.ones((4, 4), bool), dep)
            for si, (sx_, sy_) in enumerate(SHIFTS[:3]):
                for rep in range(2):
                    y, x = f_px.pop()
                    mvx, _ = aim(x, bx + sx_, w); mvy, _ = aim(y, by + sy_, h)
                    cs = 100 * fi + 10 * si + rep
                    set_pixel(y, x, "F", cs, mvx=mvx, mvy=mvy, mesh=mid, depth=d_far if far else None)
                    Fs.append((y, x, cs, int(far), s))
            fi += 1
    for rep in range(24):                                       # the current pixel itself is sky
        y, x = f_px.pop()
        C["depth"][y, x] = 1.0
        C["gb2"][y, x] = 0; C["gb3"][y, x] = 0; C["gb3"][y, x, 3] = f16bits(-1.0)
        family[y, x], case[y, x] = FAMILY["F"], 9000 + rep
        Fs.append((y, x, 9000 + rep, 2, 0))
    info["F"] = np.array(Fs, dtype=[("y", int), ("x", int), ("case", int), ("kind", int), ("sky_taps", int)])
    info["family"], info["case"] = family, case
    mv = np.concatenate([f16val(C["gb2"][..., 2:]).ravel(), f16val(H["gb2"][..., 2:]).ravel()])
    assert np.isfinite(mv).all() and np.abs(mv).max() <= 2.0
    assert all(np.isfinite(G["depth"]).all() for G in (H, C))
    return H, C, info


def reflections_variant(gb, checker=False):
    """family G: every surface pixel a mirror (roughness 0.03); checker: curvature exactly 0 / 0.5 in a checkerboard"""
    g = {k: v.copy() for k, v in gb.items()}
    geo = g["depth"] != 1.0
    g["gb3"][..., 0][geo] = f16bits(0.03)
    if checker:
        h, w = geo.shape
        board = (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)
        g["gb3"][..., 1][geo & board] = f16bits(0.5)
        g["gb3"][..., 1][geo & ~board] = 0
    return g


def describe(info, y, x):
    """what the pixel (x, y) of frame C was aimed at, for a failing test's message"""
    fam = {v: k for k, v in FAMILY.items()}[int(info["family"][y, x])]
    s = f"pixel ({x}, {y}) family {fam} case {int(info['case'][y, x])}"
    if fam in "DE" and fam != "none":
        r = info[fam][(info[fam]["y"] == y) & (info[fam]["x"] == x)]
        if len(r):
            s += f" ({'sparse' if r[0]['sparse'] else 'dense'}, " + (f"ladder offset {r[0]['ulp']} ulp, tilt {r[0]['tilt']})" if fam == "D" else f"cos^2 - 0.1 = {r[0]['dist']:+.3e})")
    return s


SIZES = [(256, 72), (200, 120), (203, 117)]
SCENES = ["cornell", "sponza_small"]
FRAME_H, FRAME_C, N_FRAMES = 2, 3, 6
_sequences = {}


def sequence(oracle, name, w, h):
    """the six-frame stream of tests/test_reproject_cases.py and tests/test_gpu_reproject_edges.py: frames 0-1 rendered (dolly 1.0), frame 2 = H,
    frame 3 = C, frames 4-5 rendered.  Returns (oracle scene, frames, info); built once per (scene, size) and never modified by its users."""
    import helpers
    key = (name, w, h)
    if key not in _sequences:
        osc = oracle.Scene(helpers.scene_data(name))
        frames = helpers.make_frames(oracle, osc, name, w, h, N_FRAMES, 1.0)
        H, C, info = craft(frames[FRAME_H]["gb"], frames[FRAME_C]["gb"], frames[FRAME_C]["ubo"])
        frames[FRAME_H]["gb"], frames[FRAME_C]["gb"] = H, C
        _sequences[key] = (osc, frames, info)
    return _sequences[key]


def reset_set(stored_length):
    """The reprojection's verdict as the temporal stages store it: they write min(32, success ? history_length + 1 : 1)
    (shadows_denoise_reprojection.comp, ao_denoise_reprojection.comp), so a pixel whose reprojected history length is 0 — every tap rejected, or
    a history texel that was sky — stores exactly 1, and an accepted ladder pixel (its history texel is a surface texel of frame H: length >= 1)
    stores >= 2.  stored_length: fp16 bit patterns."""
    return np.asarray(stored_length, np.uint16).view(np.float16).astype(np.float32) == 1.0
